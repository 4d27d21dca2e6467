"""RPN training from boxes only: anchor targets, sampling, and the two RPN losses on the device (csrc/rpn_train.hip).

Reference: lib/roi_data/rpn.py:120-279 (_get_rpn_blobs, a host step per sample there) and lib/modeling/rpn_heads.py:140-170
(single_scale_rpn_losses, sigmoid branch) with lib/utils/net.py:15-32.  Single-scale RPN only; DESIGN ("RPN training targets") lists
the quirks kept, the sampling contract and what is not here."""
import math

import numpy as np
import torch

from . import ops
from .config import generate_anchors_3d

__all__ = ["RpnTrainCfg", "RpnTargets", "rpn_targets", "rpn_losses"]


class RpnTrainCfg:
    """The TRAIN / RPN keys the step reads; defaults = the nuclei YAML merged over lib/core/config.py."""

    def __init__(self, **kw):
        self.stride = 8                                     # RPN.STRIDE
        self.sizes = (10, 27, 33, 38, 42, 46, 50)           # RPN.SIZES
        self.aspect_ratios = [[1.0, 0.5], [0.5, 0.5], [2., 0.5], [0.2, 0.5], [3., 2.]]   # RPN.ASPECT_RATIOS
        self.max_size = 256                                 # TRAIN.MAX_SIZE
        self.coarsest_stride = 32                           # FPN.COARSEST_STRIDE (config.py:703; sizes the anchor field, data_utils.py:69-72)
        self.batch_per_im = 64                              # TRAIN.RPN_BATCH_SIZE_PER_IM
        self.fg_fraction = 0.5                              # TRAIN.RPN_FG_FRACTION (config.py:132)
        self.positive_overlap = 0.5                         # TRAIN.RPN_POSITIVE_OVERLAP
        self.negative_overlap = 0.3                         # TRAIN.RPN_NEGATIVE_OVERLAP
        self.straddle_thresh = 0                            # TRAIN.RPN_STRADDLE_THRESH (config.py:151); < 0 keeps every anchor
        unknown = sorted(set(kw) - set(self.__dict__))
        if unknown:
            raise TypeError("RpnTrainCfg: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(sorted(self.__dict__))))
        self.__dict__.update(kw)

    @staticmethod
    def nuclei(**kw):
        return RpnTrainCfg(**kw)

    @staticmethod
    def soma(**kw):
        d = dict(stride=4, sizes=(10, 12, 14, 16, 18, 20, 22, 24, 28, 30, 34, 36, 38, 40), aspect_ratios=[[1.0, 1.0]], batch_per_im=128,
                 positive_overlap=0.4, negative_overlap=0.2)
        d.update(kw)
        return RpnTrainCfg(**d)

    @property
    def cell_anchors(self):
        return generate_anchors_3d(self.stride, self.sizes, self.aspect_ratios)

    @property
    def num_anchors(self):
        return len(self.sizes) * len(self.aspect_ratios)

    @property
    def field_size(self):                                   # data_utils.py:69-72
        m = self.coarsest_stride * math.ceil(self.max_size / float(self.coarsest_stride))
        return int(math.ceil(m / float(self.stride)))

    @property
    def num_fg(self):                                       # rpn.py:189
        return int(self.fg_fraction * self.batch_per_im)


class RpnTargets:
    """One image's sampled anchors, all on the device.  Indices are int64 "wide" indices a * F^3 + (z F + y) F + x into the
    [A, F, F, F] blob of rpn.py:260-261, ascending, -1 beyond the count.
      fg_index [num_fg], bg_index [batch_per_im]   anchors labelled 1 / 0
      target_index [num_fg], targets [num_fg, 6]   the fg set as sampled before the bg draws, and its regression targets
      counts [8]   #fg, #bg, #target rows, num_examples, inside anchors, fg before sampling, bg candidates, bg draws"""

    def __init__(self, fg_index, bg_index, target_index, targets, counts, num_anchors, field_size):
        self.fg_index, self.bg_index, self.target_index, self.targets, self.counts = fg_index, bg_index, target_index, targets, counts
        self.num_anchors, self.field_size = num_anchors, field_size

    @property
    def num_examples(self):
        return self.counts[3]

    def wide(self):
        """The reference's dense blobs: rpn_labels_int32_wide [1,A,F,F,F] and rpn_bbox_targets_wide / rpn_bbox_inside_weights_wide /
        rpn_bbox_outside_weights_wide [1,6A,F,F,F]."""
        return ops.rpn_target_blobs(self.fg_index, self.bg_index, self.target_index, self.targets, self.counts, self.num_anchors,
                                    self.field_size)

    def numpy(self):
        """Host copies trimmed to their counts (synchronises): dict of fg_index, bg_index, target_index, targets, counts."""
        c = self.counts.cpu().numpy()
        return dict(fg_index=self.fg_index.cpu().numpy()[:c[0]], bg_index=self.bg_index.cpu().numpy()[:c[1]],
                    target_index=self.target_index.cpu().numpy()[:c[2]], targets=self.targets.cpu().numpy()[:c[2]], counts=c)


def _boxes(b, device):
    if b is None:
        return None
    if not torch.is_tensor(b):
        b = torch.from_numpy(np.ascontiguousarray(b, np.float32).reshape(-1, 6)).to(device)
    return b.reshape(-1, 6)


def rpn_targets(gt_boxes, im_size, cfg, seed, dc_boxes=None, device="cuda"):
    """Labels, samples and regression targets of one image, on the device and without a host round trip.

    gt_boxes / dc_boxes: NumPy or CUDA fp32 [K, 6] (x1, y1, z1, x2, y2, z2); im_size = (slices, height, width); cfg: RpnTrainCfg.
    The result is a pure function of the inputs and the 64-bit `seed` (bit-identical run to run): the reference draws from
    numpy.random here, this draws from a counter hash of the seed (consecutive seeds give unrelated draws: count them up per image and step).

    No ground-truth boxes: the reference raises NameError (`anchor_to_gt_max` is unbound, rpn.py:202).  Here it means "maximum overlap
    0 everywhere": no fg, and every inside anchor that no don't-care box excludes is a bg candidate."""
    if torch.is_tensor(gt_boxes):
        device = gt_boxes.device
    gt, dc = _boxes(gt_boxes, device), _boxes(dc_boxes, device)
    out = ops.rpn_target_sets(cfg.cell_anchors, cfg.field_size, cfg.stride, gt, dc, im_size, cfg.straddle_thresh, cfg.positive_overlap,
                              cfg.negative_overlap, cfg.batch_per_im, cfg.num_fg, seed)
    return RpnTargets(*out, num_anchors=cfg.num_anchors, field_size=cfg.field_size)


class _RpnLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, pred, field_size, fg, bg, tix, tg, counts):
        losses, gx, gp = ops.rpn_loss_grad(logits, pred, field_size, fg, bg, tix, tg, counts)
        ctx.save_for_backward(gx, gp)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        gx, gp = ctx.saved_tensors
        return gx * g_cls, gp * g_box, None, None, None, None, None, None


def rpn_losses(rpn_cls_logits, rpn_bbox_pred, targets):
    """(loss_rpn_cls, loss_rpn_bbox) of single_scale_rpn_losses (sigmoid branch) for rpn_cls_logits [B,A,s,h,w] and rpn_bbox_pred
    [B,6A,s,h,w]; `targets`: one RpnTargets per image (or a single one for B = 1).  One launch computes both losses and both gradients;
    backward scales the stored gradients by the incoming scalars."""
    ts = [targets] if isinstance(targets, RpnTargets) else list(targets)
    if len(ts) != rpn_cls_logits.shape[0]:
        raise ops.M3DError("rpn_losses: %d target sets for a batch of %d" % (len(ts), rpn_cls_logits.shape[0]))
    if any(t.field_size != ts[0].field_size or t.num_anchors != ts[0].num_anchors for t in ts):
        raise ops.M3DError("rpn_losses: the target sets of a batch must share one anchor field")
    cap_fg, cap_bg = max(t.fg_index.shape[0] for t in ts), max(t.bg_index.shape[0] for t in ts)

    def stack(name, cap, fill):       # images sampled with different batch sizes: rows beyond an image's count are never read
        rows = [getattr(t, name) for t in ts]
        return torch.stack([r if r.shape[0] == cap else torch.cat([r, r.new_full((cap - r.shape[0],) + tuple(r.shape[1:]), fill)]) for r in rows])
    return _RpnLoss.apply(rpn_cls_logits, rpn_bbox_pred, ts[0].field_size, stack("fg_index", cap_fg, -1), stack("bg_index", cap_bg, -1),
                          stack("target_index", cap_fg, -1), stack("targets", cap_fg, 0), torch.stack([t.counts for t in ts]))
