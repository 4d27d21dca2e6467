"""m3d — host-side Python over libm3d.so (hand-written HIP for gfx950, C ABI in include/m3d.h).

PyTorch is used for device memory, streams and torch.distributed only.  There is NO CPU fallback: importing
an op without the built library, or calling one without a GPU tensor, raises.
"""
from . import _lib  # noqa: F401
from .ops import *  # noqa: F401,F403
from .train import (RpnTrainCfg, RpnTargets, rpn_targets, rpn_losses, BoxHeadTrainCfg, BoxHeadTargets, box_head_targets,  # noqa: E402,F401
                    box_head_losses, bn_stats, batch_norm_relu, DsnBody, MaskTrainCfg, MaskTargets, mask_targets, mask_losses,
                    MaskHead, upconv3d_2x, ConvBoxHead)
from .solver import SolverCfg, Solver, save_ckpt, load_ckpt  # noqa: E402,F401
from .data import SampleCfg, Annotations, read_soma_annotations, read_nuclei_annotations, epoch_order, TrainSet, Batch  # noqa: E402,F401
from .peaks import peak_stimulation_3d, peak_stimulation_3d_dev, PeakStimulation  # noqa: E402,F401
