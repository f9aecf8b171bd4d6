"""data/dataset.py of the reference -> adam-dehaze_amd.data (device-resident 8-bit cache, HIP batch assembly)."""
from adam_dehaze_amd.data import FolderDataset, folder_index, folder_loader  # noqa: F401


def get_dataloader(config, split="train"):
    """data/dataset.py:233-249: the loader of one split.  Where the reference returns a torch DataLoader, this returns the
    epoch callable of `adam_dehaze_amd.data.folder_loader` (`loader(epoch)` iterates the batch dicts; the drivers take it as
    `train_loader=` / `val_loader=` / `test_loader=`), on `config['device']`.  Raises when the configured path holds no image
    folders: the reference's `os.listdir` does, too."""
    loader = folder_loader(config, split, config.get("device", "cuda"))
    if loader is None:
        raise FileNotFoundError(f"no image folders for the {split} split under the configured dataset path")
    return loader
