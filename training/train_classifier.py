"""training/train_classifier.py of the reference -> adam-dehaze_amd.train (HIP engine)."""
from adam_dehaze_amd.train import evaluate_classifier, train_classifier  # noqa: F401
