"""dpot_amd - MI355X-native (gfx950 / CDNA4) implementation of the DPOT auto-regressive forward/backward step.

    from dpot_amd import DPOTNet            # drop-in for models/dpot.py::DPOTNet of HaoZhongkai/DPOT
    from dpot_amd.train import FlatParams, FusedAdam, FusedLamb, train_step, GraphedTrainStep
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd import StepMetrics, cls_ce_loss     # device-side training metrics, the dataset-classification loss
    from dpot_amd import rollout_eval, GraphedRollout, refill_mask, spectral_resize   # evaluation at any data resolution
    from dpot_amd import RolloutEvaluator              # the PDEBench metric set of the reference's Evaluator, on the device
    from dpot_amd import DPOTNet3D, load_3d_components_from_2d   # 3-D fine-tuning from a pretrained 2-D checkpoint
    from dpot_amd import DeviceBatcher3D, resize_pad_window3, target_mask3   # the 3-D input pipeline on the device
    from dpot_amd import CDPOTNet           # drop-in for models/dpot_res.py::CDPOTNet (anti-aliased embed and output stages)
    from dpot_amd import FNO2d              # drop-in for models/fno.py::FNO2d, the baseline (truncated-DFT and per-mode mixing kernels)
    from dpot_amd import FNO3d              # drop-in for models/fno.py::FNO3d, the 3-D baseline of finetune3d.py
    from dpot_amd import Resized3D, spectral_resize3, resize3_plan   # 3-D rollouts at any data resolution
    from dpot_amd import UNet               # drop-in for models/unet.py::UNet (n_dim = 2): 3x3 convolution, BatchNorm and pooling kernels

The compute path is libdpot_hip.so (hand-written HIP kernels behind the C ABI in include/dpot_hip.h).
"""
from .model import DPOTNet  # noqa: F401
from .model3d import DPOTNet3D  # noqa: F401
from .model_c import CDPOTNet  # noqa: F401
from .model_fno import FNO2d  # noqa: F401
from .model_fno3d import FNO3d  # noqa: F401
from .model_unet import UNet  # noqa: F401
from . import _lib  # noqa: F401
from .functional import ClsCEFn, cls_ce_loss  # noqa: F401
from .train import StepMetrics  # noqa: F401
from .infer import GraphedRollout, Resized3D, RolloutEvaluator, load_3d_components_from_2d, refill_mask, rollout_eval  # noqa: F401
from .ops import ResizePlan, spectral_resize, spectral_resize_matrices  # noqa: F401
from .ops import Resize3Plan, resize3_plan, spectral_resize3  # noqa: F401
from .data import DeviceBatcher3D, resize_pad_window3, target_mask3  # noqa: F401

__version__ = "0.3.0"
__all__ = ["DPOTNet", "StepMetrics", "ClsCEFn", "cls_ce_loss", "GraphedRollout", "rollout_eval", "refill_mask",
           "spectral_resize", "spectral_resize_matrices", "ResizePlan", "RolloutEvaluator", "DPOTNet3D",
           "load_3d_components_from_2d", "DeviceBatcher3D", "resize_pad_window3", "target_mask3", "CDPOTNet", "FNO2d",
           "FNO3d", "Resized3D", "spectral_resize3", "resize3_plan", "Resize3Plan", "UNet"]
