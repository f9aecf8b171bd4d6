"""training/loss.py of the reference -> adam-dehaze_amd (HIP kernels)."""
from adam_dehaze_amd.loss import (  # noqa: F401
    ContentLoss, DehazingLoss, FrequencyLoss, JointLoss, MSSSIMLoss, SSIMLoss, frequency_l1, get_dehazing_loss, get_joint_loss,
    ms_ssim_per_image, ssim_per_image)
