"""Reference import paths (`data.*`) resolved to the MI355X implementation in adam-dehaze_amd/."""
