"""Native (gfx950 HIP) operators with autograd and CPU reference fallbacks."""
from .averaging import AveragedModel  # noqa: F401
from .clip import GradClipper, clip_grad_norm_, clip_grad_value_  # noqa: F401
from .flat import FlatParameters, contiguous_span  # noqa: F401
from .fused_step import FusedMLPStep  # noqa: F401
from .linear import Linear, gemm, linear  # noqa: F401
from .loss import CrossEntropyLoss, MSELoss, cross_entropy, mse_loss  # noqa: F401
from .lr_scheduler import (ConstantLR, CosineAnnealingLR, ExponentialLR, LinearLR, MultiStepLR,  # noqa: F401
                           PolynomialLR, SequentialLR, StepLR)
from .metrics import ClassificationMeter, classification_rows  # noqa: F401
from .norm import BatchNorm2d, SyncBatchNorm  # noqa: F401
from .optim import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, layerwise_param_groups  # noqa: F401
