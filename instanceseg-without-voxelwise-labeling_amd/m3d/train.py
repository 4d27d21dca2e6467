"""RPN training from boxes only: anchor targets, sampling, and the two RPN losses on the device (csrc/rpn_train.hip).

Reference: lib/roi_data/rpn.py:120-279 (_get_rpn_blobs, a host step per sample there) and lib/modeling/rpn_heads.py:140-170
(single_scale_rpn_losses, sigmoid branch) with lib/utils/net.py:15-32.  Single-scale RPN only; DESIGN ("RPN training targets") lists
the quirks kept, the sampling contract and what is not here.

Box head from proposals and boxes (csrc/box_head_train.hip): proposal labelling, fg / bg sampling, regression targets and the softmax /
smooth-L1 losses.  Reference: lib/modeling/generate_proposal_labels_3d.py, lib/datasets/nuclei_dataset.py:429-547,
lib/roi_data/fast_rcnn.py:129-248, lib/modeling/fast_rcnn_heads.py:50-66; DESIGN ("Box-head training targets").

BatchNorm3d on batch statistics (csrc/bn_train.hip): bn_stats, the fused batch_norm_relu (BatchNorm3d -> ReLU -> MaxPool3d(2,2), forward
and backward) and DsnBody, the reference's body on it.  Reference: lib/modeling/DSN.py:15-68 under maskRCNN.train(); DESIGN ("BatchNorm
training").

Mask branch from the sampled fg RoIs (csrc/mask_train.hip): per RoI the M^3 target of its ground-truth sphere or labelled instance, the
sigmoid cross entropy over the labelled voxels, and MaskHead, the reference's head under its parameter names.  Reference:
lib/roi_data/mask_rcnn.py:34-135, lib/utils/segms.py:120-225, lib/modeling/mask_rcnn_heads.py:20-68, 90-99, 132-193; DESIGN ("Mask-branch
training targets")."""
import math

import numpy as np
import torch

from . import ops
from .config import generate_anchors_3d

__all__ = ["RpnTrainCfg", "RpnTargets", "rpn_targets", "rpn_losses", "BoxHeadTrainCfg", "BoxHeadTargets", "box_head_targets", "box_head_losses",
           "bn_stats", "batch_norm_relu", "DsnBody", "MaskTrainCfg", "MaskTargets", "mask_targets", "mask_losses", "MaskHead"]


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


class BoxHeadTrainCfg:
    """The TRAIN / MODEL keys the box-head step reads; defaults = the nuclei YAML merged over lib/core/config.py."""

    def __init__(self, **kw):
        self.batch_per_im = 64                              # TRAIN.BATCH_SIZE_PER_IM
        self.fg_fraction = 0.25                             # TRAIN.FG_FRACTION (config.py:65)
        self.fg_thresh = 0.4                                # TRAIN.FG_THRESH
        self.bg_thresh_hi = 0.4                             # TRAIN.BG_THRESH_HI
        self.bg_thresh_lo = 0.0                             # TRAIN.BG_THRESH_LO (config.py:73)
        self.num_classes = 2                                # MODEL.NUM_CLASSES
        self.bbox_reg_weights = (10., 10., 10., 5., 5., 5.)   # MODEL.BBOX_REG_WEIGHTS
        self.cls_agnostic_bbox_reg = False                  # MODEL.CLS_AGNOSTIC_BBOX_REG: True is refused (DESIGN)
        unknown = sorted(set(kw) - set(self.__dict__))
        if unknown:
            raise TypeError("BoxHeadTrainCfg: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(sorted(self.__dict__))))
        self.__dict__.update(kw)

    @staticmethod
    def nuclei(**kw):
        return BoxHeadTrainCfg(**kw)

    @staticmethod
    def soma(**kw):
        d = dict(batch_per_im=128)
        d.update(kw)
        return BoxHeadTrainCfg(**d)

    @property
    def fg_per_im(self):                                    # fast_rcnn.py:134
        return int(np.round(self.fg_fraction * int(self.batch_per_im)))


class BoxHeadTargets:
    """The sampled box-head rows of B images, on the device, each image padded to batch = BATCH_SIZE_PER_IM (fg rows ascending in
    roidb row, then bg rows ascending; roidb row r < K = ground-truth box r, r >= K = proposal r - K):
      rows int64 [B,batch] (-1 beyond the count), labels int32 [B,batch] (class / 0 / -1), rois fp32 [B,batch,6], targets fp32 [B,batch,6]
      counts int64 [B,8]   rows, fg, bg sampled; fg, bg candidates; crowd gt rows; non-crowd gt boxes; proposals"""

    def __init__(self, rows, labels, rois, targets, counts, cfg):
        self.rows, self.labels, self.rois, self.targets, self.counts, self.cfg = rows, labels, rois, targets, counts, cfg

    @property
    def rois7(self):
        """fp32 [B batch, 7] for RoIAlign: the batch index in column 0; a padding row is a zero box on image 0."""
        B, batch = self.labels.shape
        index = torch.arange(B, device=self.labels.device, dtype=torch.float32)[:, None] * (self.labels >= 0).float()
        return torch.cat([index[:, :, None], self.rois], 2).reshape(B * batch, 7)

    def blobs(self):
        """The reference's five blobs over the padded rows (fast_rcnn.py:186-191): labels_int32 [N], rois [N,7], bbox_targets,
        bbox_inside_weights, bbox_outside_weights [N, 6 NUM_CLASSES], N = B batch; a padding row is label -1 and zeros."""
        bt, iw, ow = ops.box_head_target_blobs(self.labels, self.targets, self.cfg.num_classes)
        return dict(labels_int32=self.labels.reshape(-1), rois=self.rois7, bbox_targets=bt, bbox_inside_weights=iw, bbox_outside_weights=ow)

    def numpy(self):
        """Host copies trimmed to their counts (synchronises): one dict of rows, labels, rois, targets, counts per image."""
        c = self.counts.cpu().numpy()
        rows, labels, rois, targets = (t.cpu().numpy() for t in (self.rows, self.labels, self.rois, self.targets))
        return [dict(rows=rows[b, :c[b, 0]], labels=labels[b, :c[b, 0]], rois=rois[b, :c[b, 0]], targets=targets[b, :c[b, 0]], counts=c[b])
                for b in range(len(c))]


def _per_image(values, gt_list, dtype, device, name, caller="box_head_targets"):
    """per-image class / crowd arrays -> one device tensor over the concatenated boxes; an image given as None takes the default"""
    if values is None:
        return None
    if len(values) != len(gt_list):
        raise ops.M3DError("%s: %s needs one entry per image" % (caller, name))
    parts = []
    for v, g in zip(values, gt_list):
        if v is None:
            v = torch.full((g.shape[0],), 1 if name == "gt_classes" else 0, dtype=dtype, device=device)
        elif not torch.is_tensor(v):
            v = torch.from_numpy(np.ascontiguousarray(v).astype(np.int64).reshape(-1)).to(device)
        if v.numel() != g.shape[0]:
            raise ops.M3DError("%s: %s has %d entries for %d boxes" % (caller, name, v.numel(), g.shape[0]))
        parts.append(v.reshape(-1).to(device=device, dtype=dtype))
    return torch.cat(parts).contiguous()


def box_head_targets(rois, num, gt_boxes, cfg, seed, gt_classes=None, gt_crowd=None):
    """Labels the proposals of B images against their ground-truth boxes, samples BATCH_SIZE_PER_IM rows per image and computes their
    regression targets, on the device and without a host round trip.

    rois fp32 [B,rows,7] and num int32 [B]: as ops.generate_proposals3d_batched returns them (CUDA).  gt_boxes: one NumPy or CUDA fp32
    [K_b,6] array per image; gt_classes / gt_crowd: None, or per image an array of K_b classes (1 .. NUM_CLASSES-1) / crowd flags (or
    None for "all 1" / "none").  seed: one 64-bit seed per image, or one base seed (image b then samples with seed + b).  The result is
    a pure function of the inputs and the seeds, bit-identical run to run.

    An image without (non-crowd) boxes: the reference raises IndexError in _sample_rois; here every proposal has overlap 0, so there is
    no fg row and the batch fills with bg rows."""
    if not torch.is_tensor(rois) or not torch.is_tensor(num) or not rois.is_cuda or not num.is_cuda:
        raise ops.M3DError("box_head_targets: rois and num must be CUDA (ROCm) tensors; there is no CPU path")
    dev = rois.device
    gts = [_boxes(g, dev) for g in gt_boxes]
    if len(gts) != rois.shape[0]:
        raise ops.M3DError("box_head_targets: %d box arrays for %d images" % (len(gts), rois.shape[0]))
    ops._need_gpu(*gts)
    off = np.concatenate([[0], np.cumsum([g.shape[0] for g in gts])]).astype(np.int32)
    gt = torch.cat([g.float() for g in gts]) if gts else torch.zeros((0, 6), device=dev)
    seeds = [int(s) for s in seed] if np.ndim(seed) else [int(seed) + b for b in range(len(gts))]
    out = ops.box_head_target_sets(rois, num, gt, off, _per_image(gt_classes, gts, torch.int32, dev, "gt_classes"),
                                   _per_image(gt_crowd, gts, torch.uint8, dev, "gt_crowd"), cfg.batch_per_im, cfg.fg_per_im, cfg.fg_thresh,
                                   cfg.bg_thresh_hi, cfg.bg_thresh_lo, cfg.bbox_reg_weights, cfg.num_classes, seeds,
                                   cfg.cls_agnostic_bbox_reg)
    return BoxHeadTargets(*out, cfg=cfg)


class _BoxHeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, pred, labels, targets, counts):
        losses, gs, gp = ops.box_head_loss_grad(score, pred, labels, targets, counts)
        ctx.save_for_backward(gs, gp)
        accuracy = losses[2]
        ctx.mark_non_differentiable(accuracy)
        return losses[0], losses[1], accuracy

    @staticmethod
    def backward(ctx, g_cls, g_box, g_acc):
        gs, gp = ctx.saved_tensors
        return gs * g_cls, gp * g_box, None, None, None


def box_head_losses(cls_score, bbox_pred, targets):
    """(loss_cls, loss_bbox, accuracy_cls) of fast_rcnn_losses for cls_score [B batch, C] and bbox_pred [B batch, 6 C] computed on
    `targets.rois7`; `targets`: the BoxHeadTargets of the minibatch.  The mean runs over the sampled rows (padding rows count nowhere and
    get zero gradients).  One launch computes the losses and both gradients; backward scales the stored gradients."""
    return _BoxHeadLoss.apply(cls_score, bbox_pred, targets.labels, targets.targets, targets.counts)


bn_stats = ops.bn_stats          # one function under both names: m3d.bn_stats(x) -> (mean, var, invstd)


class _BatchNormRelu(torch.autograd.Function):
    """Saves x, mean, invstd and the pool arg-max - not y: the backward recomputes z from x by the forward's own expression."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, training, momentum, eps, relu, pool):
        Cn = x.shape[1]
        w = weight.detach() if weight is not None else torch.ones((Cn,), dtype=torch.float32, device=x.device)
        b = bias.detach() if bias is not None else torch.zeros((Cn,), dtype=torch.float32, device=x.device)
        if training:
            mean, var, invstd = ops.bn_stats(x, eps, running_mean, running_var, momentum)   # the same launch moves the running statistics
        else:
            mean, invstd = running_mean.detach(), ops.bn_invstd(running_var.detach(), eps)
        out = ops.bn_apply(x, mean, invstd, w, b, relu, pool)
        y, argmax = out if pool else (out, None)
        ctx.save_for_backward(x, mean, invstd, w, b, argmax)
        ctx.cfg = (bool(training), bool(relu), bool(pool), weight is not None, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, mean, invstd, w, b, argmax = ctx.saved_tensors
        training, relu, pool, has_w, has_b = ctx.cfg
        gx, gw, gb = ops.bn_backward(x, mean, invstd, w, b, gy.contiguous(), argmax, relu, pool, training)
        return (gx if ctx.needs_input_grad[0] else None, gw if has_w and ctx.needs_input_grad[1] else None,
                gb if has_b and ctx.needs_input_grad[2] else None, None, None, None, None, None, None, None)


def batch_norm_relu(x, weight, bias, running_mean=None, running_var=None, training=True, momentum=0.1, eps=1e-5, relu=True, pool=False):
    """BatchNorm3d [-> ReLU] [-> MaxPool3d(2, 2)] of a CUDA fp32 [N,C,D,H,W] tensor in one pass over x after the statistics, with its
    backward (two passes).  training: batch statistics, and the running statistics (if given) are updated in place as
    torch.nn.BatchNorm3d updates them (rm <- (1 - m) rm + m mean, rv <- (1 - m) rv + m var n / (n - 1)); else the running statistics
    normalise.  weight / bias may be None (1 / 0).  With pool only the pooled tensor is ever stored (D, H, W must be even)."""
    ts = [t for t in (x, weight, bias, running_mean, running_var) if t is not None]
    if not all(torch.is_tensor(t) and t.is_cuda for t in ts):
        raise ops.M3DError("batch_norm_relu: needs CUDA (ROCm) tensors; there is no CPU path")
    if x.dtype != torch.float32 or x.dim() != 5:
        raise ops.M3DError("batch_norm_relu: x must be fp32 [N,C,D,H,W]")
    if not training and (running_mean is None or running_var is None):
        raise ops.M3DError("batch_norm_relu: evaluation mode needs running_mean and running_var")
    if training and x.numel() // max(x.shape[1], 1) < 2:
        raise ops.M3DError("batch_norm_relu: batch statistics need more than one value per channel")
    if pool and any(int(v) % 2 for v in x.shape[2:]):
        raise ops.M3DError("batch_norm_relu: pool needs even depth, height and width, got %s" % (tuple(x.shape[2:]),))
    momentum = 0.0 if momentum is None else float(momentum)
    return _BatchNormRelu.apply(x.contiguous(), weight, bias, running_mean, running_var, bool(training), momentum, float(eps), bool(relu),
                                bool(pool))


class DsnBody(torch.nn.Module):
    """dsn_body of lib/modeling/DSN.py:15-68 with its parameter and buffer names (conv1a, bn1a, conv2a, ... bn4b), so that state dicts
    pass both ways: F.conv3d (libm3d's kernels where m3d.compat routes it), then the fused batch_norm_relu; the reference's pool1 / pool2 /
    pool3 are fused into bn1a / bn2b / bn3b.  Follows self.training: batch statistics in train(), running statistics in eval().
    width: channels of conv1a (the reference has 32); stride 4 ends after bn3b, as RPN.STRIDE 4 does there."""

    def __init__(self, stride=8, width=32):
        super().__init__()
        if stride not in (4, 8):
            raise ValueError("DsnBody: stride 4 or 8")
        w = int(width)
        plan = [("1a", 1, w, 5, True), ("2a", w, 2 * w, 3, False), ("2b", 2 * w, 2 * w, 3, True), ("3a", 2 * w, 4 * w, 3, False),
                ("3b", 4 * w, 4 * w, 3, stride == 8)]
        if stride == 8:
            plan += [("4a", 4 * w, 8 * w, 3, False), ("4b", 8 * w, 8 * w, 3, False)]
        self.layers = tuple((name, pool) for name, _, _, _, pool in plan)
        for name, cin, cout, k, _ in plan:
            conv = torch.nn.Conv3d(cin, cout, k, 1, k // 2, bias=True)
            torch.nn.init.normal_(conv.weight, std=0.01)           # DSN.py:44-53
            torch.nn.init.constant_(conv.bias, 0.0)
            setattr(self, "conv" + name, conv)
            setattr(self, "bn" + name, torch.nn.BatchNorm3d(cout, momentum=0.001, affine=True))
        self.dim_out, self.spatial_scale = plan[-1][2], 1.0 / stride

    def forward(self, x):
        for name, pool in self.layers:
            conv, bn = getattr(self, "conv" + name), getattr(self, "bn" + name)
            x = torch.nn.functional.conv3d(x, conv.weight, conv.bias, 1, conv.padding)
            if self.training:
                bn.num_batches_tracked.add_(1)
            x = batch_norm_relu(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, self.training, bn.momentum, bn.eps, True, pool)
        return x


class MaskTrainCfg:
    """The MRCNN / TRAIN / MODEL keys the mask step reads; defaults = the nuclei YAML merged over lib/core/config.py."""

    def __init__(self, **kw):
        self.resolution = 14                                # MRCNN.RESOLUTION
        self.anno_type = "mask"                             # MRCNN.ANNO_TYPE: 'mask' (label volume + markers) or 'spot' (spheres)
        self.cls_specific = False                           # MRCNN.CLS_SPECIFIC_MASK
        self.weight_loss_mask = 1.0                         # MRCNN.WEIGHT_LOSS_MASK
        self.in_size = (64, 256, 256)                       # TRAIN.IN_SIZE: clips the boxes of the spots (segms.py:214)
        self.num_classes = 2                                # MODEL.NUM_CLASSES
        self.roi_xform_resolution = 7                       # MRCNN.ROI_XFORM_RESOLUTION
        self.sampling_ratio = 2                             # MRCNN.ROI_XFORM_SAMPLING_RATIO
        self.dim_reduced = 256                              # MRCNN.DIM_REDUCED
        self.num_convs = 3                                  # MRCNN.ROI_MASK_HEAD: mask_rcnn_fcn_head_v1up3convs
        self.dilation = 1                                   # MRCNN.DILATION: both shipped YAMLs set 1 (lib/core/config.py:767 defaults to 2)
        unknown = sorted(set(kw) - set(self.__dict__))
        if unknown:
            raise TypeError("MaskTrainCfg: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(sorted(self.__dict__))))
        self.__dict__.update(kw)
        if self.anno_type not in ("mask", "spot"):
            raise ValueError("MaskTrainCfg: anno_type is 'mask' or 'spot'")
        if self.dilation not in (1, 2):
            raise ValueError("MaskTrainCfg: dilation is 1 or 2 (the library's dilated 3^3 conv is dilation 2 only)")

    @staticmethod
    def nuclei(**kw):
        return MaskTrainCfg(**kw)

    @staticmethod
    def soma(**kw):
        d = dict(anno_type="spot", num_convs=4)
        d.update(kw)
        return MaskTrainCfg(**d)

    @property
    def mask_classes(self):
        return int(self.num_classes) if self.cls_specific else 1


class MaskTargets:
    """The mask targets of the fg rows of B images, on the device, each image padded to fg_per_im rows:
      masks int32 [B,fg_per_im,Cm M^3] (1 / 0, -1 = ignore; a padding row is all -1), rois fp32 [B,fg_per_im,6] (0 beyond the count),
      assign int32 [B,fg_per_im] (the object's index within its image, -1 beyond), counts int64 [B,4] = fg rows, positive voxels,
      labelled voxels, 0.  `labels` are the box-head labels [B,batch] the targets were made for."""

    def __init__(self, masks, rois, assign, counts, labels, cfg):
        self.masks, self.rois, self.assign, self.counts, self.labels, self.cfg = masks, rois, assign, counts, labels, cfg

    @property
    def rois7(self):
        """fp32 [B fg_per_im, 7] for RoIAlign: the batch index in column 0; a padding row is a zero box on image 0."""
        B, F = self.assign.shape
        live = torch.arange(F, device=self.assign.device)[None, :] < self.counts[:, :1]
        index = torch.arange(B, device=self.assign.device, dtype=torch.float32)[:, None] * live.float()
        return torch.cat([index[:, :, None], self.rois], 2).reshape(B * F, 7)

    def blobs(self):
        """The reference's three blobs over the padded rows (mask_rcnn.py:110-112): mask_rois [B fg_per_im, 7], roi_has_mask_int32
        [B batch] = labels > 0, masks_int32 [B fg_per_im, Cm M^3]."""
        ops._need_gpu(self.masks, self.labels)
        return dict(mask_rois=self.rois7, roi_has_mask_int32=(self.labels > 0).to(torch.int32).reshape(-1),
                    masks_int32=self.masks.reshape(-1, self.masks.shape[2]))

    def numpy(self):
        """Host copies trimmed to their counts (synchronises): one dict of masks, rois, assign, counts per image."""
        c = self.counts.cpu().numpy()
        masks, rois, assign = (t.cpu().numpy() for t in (self.masks, self.rois, self.assign))
        return [dict(masks=masks[b, :c[b, 0]], rois=rois[b, :c[b, 0]], assign=assign[b, :c[b, 0]], counts=c[b]) for b in range(len(c))]


def _objects(values, width, dtype, device, name, B):
    """per-image object arrays (NumPy or CUDA) -> (list of device tensors [K_b, width], host offsets)"""
    if values is None or len(values) != B:
        raise ops.M3DError("mask_targets: %s needs one array per image" % name)
    out = []
    for v in values:
        if not torch.is_tensor(v):
            v = torch.from_numpy(np.ascontiguousarray(v).astype(np.float32 if dtype == torch.float32 else np.int64)).to(device)
        out.append(v.reshape(-1, width).to(device=device, dtype=dtype))
    return out, np.concatenate([[0], np.cumsum([o.shape[0] for o in out])]).astype(np.int32)


def mask_targets(box_targets, cfg, spots=None, gt_boxes=None, markers=None, labels=None, gt_classes=None, gt_crowd=None):
    """The mask targets of the fg rows of `box_targets` (the BoxHeadTargets of the minibatch), on the device and without a host round trip.

    cfg: MaskTrainCfg.  anno_type 'spot': spots = per image a NumPy or CUDA fp32 [K_b,4] array (x, y, z, r) in tile coordinates
    (Batch.gt_spots).  anno_type 'mask': gt_boxes = per image the roidb boxes [K_b,6], markers = per image the K_b marker ids, labels =
    per image a CUDA uint16 or int32 label volume [D,H,W] in tile coordinates.  The objects are those box_head_targets saw, in the same
    order; gt_classes / gt_crowd as there.  A RoI takes the object whose box (for spots: spots_to_boxes of the sphere, not the roidb box)
    overlaps it most, the first among equals.  Bit-identical run to run.  The target is "resize > 0" with the reference's resize carried
    out in fp64: where the reference's fp32 resize underflows (extents such as 18, 34, 58) it can hold a few voxels more (DESIGN)."""
    T = box_targets
    if not torch.is_tensor(T.labels) or not T.labels.is_cuda:
        raise ops.M3DError("mask_targets: the box-head targets must live on the device; there is no CPU path")
    dev, B = T.labels.device, T.labels.shape[0]
    if (cfg.anno_type == "spot") != (spots is not None) or (cfg.anno_type == "mask") != (gt_boxes is not None):
        raise ops.M3DError("mask_targets: anno_type '%s' takes %s" % (cfg.anno_type, "spots" if cfg.anno_type == "spot" else
                                                                      "gt_boxes, markers and labels"))
    fg_per_im = T.cfg.fg_per_im
    if cfg.anno_type == "spot":
        objs, off = _objects(spots, 4, torch.float32, dev, "spots", B)
        kw = dict(spots=torch.cat(objs).contiguous() if objs else None, in_size=cfg.in_size)
    else:
        objs, off = _objects(gt_boxes, 6, torch.float32, dev, "gt_boxes", B)
        mk, off2 = _objects(markers, 1, torch.int32, dev, "markers", B)
        if not np.array_equal(off, off2) or labels is None or len(labels) != B:
            raise ops.M3DError("mask_targets: one marker per box and one label volume per image")
        kw = dict(gt=torch.cat(objs).contiguous(), markers=torch.cat(mk).reshape(-1).contiguous(), volumes=list(labels))
    out = ops.mask_target_sets(T.labels, T.rois, T.counts, off, fg_per_im, cfg.resolution, cfg.num_classes, cfg.cls_specific,
                               gt_classes=_per_image(gt_classes, objs, torch.int32, dev, "gt_classes", "mask_targets"),
                               gt_crowd=_per_image(gt_crowd, objs, torch.uint8, dev, "gt_crowd", "mask_targets"), **kw)
    return MaskTargets(*out, labels=T.labels, cfg=cfg)


class _MaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, masks, weight):
        loss, _, gx = ops.mask_loss_grad(pred, masks, weight)
        ctx.save_for_backward(gx)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        gx, = ctx.saved_tensors
        return gx * g, None, None


def mask_losses(mask_pred, targets):
    """loss_mask of mask_rcnn_losses for mask_pred [B fg_per_im, Cm, M, M, M] computed on `targets.rois7`; `targets`: the MaskTargets of
    the minibatch.  The mean runs over the labelled voxels (padding rows and, with cls_specific, the other classes' blocks count nowhere
    and get zero gradients; no labelled voxel at all: loss 0, where the reference divides 0 by 0).  One call computes the loss and the
    gradient; backward scales the stored gradient."""
    if not torch.is_tensor(mask_pred) or not mask_pred.is_cuda:
        raise ops.M3DError("mask_losses: mask_pred must be a CUDA (ROCm) tensor; there is no CPU path")
    return _MaskLoss.apply(mask_pred, targets.masks, float(targets.cfg.weight_loss_mask))


class _UpConv3d2x(torch.autograd.Function):
    """ConvTranspose3d(kernel 2, stride 2, padding 0) (+ ReLU) on csrc/upconv3d.hip.  With relu the forward's own output is saved and
    handed to both backward kernels as the mask: no ReLU-backward pass over the 2x tensor.  Only the gradients autograd asks for are
    computed; the bias gradient comes out of the wgrad launch.  Each backward direction runs where conv_plan.upconv_backward_kernel says
    (compat.set_upconv_backward: csrc/upconv3d_bwd_f16.hip for the directions it routes, gy swept once for both)."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, f16=False):
        b = None if bias is None else bias.detach()
        up = None
        if f16 and ops.UpConvF16.supported(weight):          # compat.set_upconv_f16: the forward alone
            from . import compat
            up = compat._packed(weight, "upconv-f16")
        ctx.x_bound = None
        if up is not None and x.shape[0] > 0 and up.supports(tuple(x.shape)):
            ctx.x_bound = ops.ZwConv3d.bound_of(x)               # the sweep UpConvF16 makes for in_max=None, kept for an f16x2 wgrad
            y = up(x, ctx.x_bound, bias=b, relu=relu)
        else:
            y = ops.upconv3d_2x_forward(x, weight.detach(), b, relu=relu)
        ctx.relu, ctx.has_bias = bool(relu), bias is not None
        ctx.save_for_backward(x, weight, y if relu else None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight, y = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = gb = None
        from . import compat, conv_plan
        want_gb = ctx.has_bias and ctx.needs_input_grad[2]
        want = {"dgrad": ctx.needs_input_grad[0], "wgrad": ctx.needs_input_grad[1] or want_gb}
        dims = (x.shape[0], x.shape[1], weight.shape[1]) + tuple(x.shape[2:])
        f16 = {d: want[d] and x.shape[0] > 0 and conv_plan.upconv_backward_kernel(d, *dims, compat._upconv_backward)
               == conv_plan.UPCONV_BACKWARD_F16X2 for d in want}
        gy_max = ops.ZwConv3d.bound_of(gy) if (f16["dgrad"] or f16["wgrad"]) else None      # one sweep, both passes
        if f16["dgrad"]:
            gx = ops.upconv3d_2x_dgrad_f16x2(gy, weight.detach(), y=y, gy_max=gy_max, w_max=compat._upconv_weight_max(weight))
        elif want["dgrad"]:
            gx = ops.upconv3d_2x_dgrad(gy, weight.detach(), y=y)
        if f16["wgrad"]:
            gw, gb = ops.upconv3d_2x_wgrad_f16x2(gy, x.detach(), y=y, gy_max=gy_max, x_max=ctx.x_bound, bias=want_gb)
        elif want["wgrad"]:
            gw, gb = ops.upconv3d_2x_wgrad(gy, x.detach(), y=y, bias=want_gb)
        if not ctx.needs_input_grad[1]:
            gw = None
        return gx, gw, gb, None, None


def upconv3d_2x(x, weight, bias=None, relu=False):
    """torch.nn.functional.conv_transpose3d(x, weight, bias, stride=2) for a [Cin,Cout,2,2,2] weight, followed by ReLU if `relu`, forward
    and backward on the library's kernels (mask_rcnn_heads.py:156,193).  x [R,Cin,D,H,W] -> [R,Cout,2D,2H,2W], fp32."""
    for t in (x, weight, bias):
        if t is not None and (not torch.is_tensor(t) or not t.is_cuda):
            raise ops.M3DError("upconv3d_2x: x, weight and bias must be CUDA (ROCm) tensors; there is no CPU path")
    from . import compat
    f16 = compat.get_upconv_f16() and compat.get_upconv() == compat.UPCONV_M3D
    return _UpConv3d2x.apply(x.contiguous(), weight.contiguous(), bias, bool(relu), bool(f16))


class MaskHead(torch.nn.Module):
    """mask_rcnn_fcn_head_v1upXconvs followed by mask_rcnn_outputs (mask_rcnn_heads.py:132-193, 20-68; conv classifier, no
    upsampling) as one module under the reference's parameter names conv_fcn.{0,2,..}, upconv, classify: its state_dict, prefixed
    Mask_Head. / Mask_Outs. by `detector_state`, is what MaskHeadM3D takes.  RoIAlign3D and the convolutions go through m3d.compat (the
    library's kernels, forward and backward).  The up-conv follows compat.set_upconv: "torch" (the default) is torch's ConvTranspose3d
    and a separate ReLU; "m3d" is upconv3d_2x with the bias and the ReLU in its epilogue and the library's dgrad / wgrad kernels behind
    it - the same module, parameters and state_dict under both.  cfg.dilation (MRCNN.DILATION) is the dilation and the padding of the 3^3
    convs; no parameter name or shape depends on it.  At dilation 2 they follow compat.set_conv_dilated: "torch" (the default) is torch's
    conv3d, "m3d" the library's dilated forward, dgrad and wgrad.  forward returns logits, as the reference does in training."""

    def __init__(self, dim_in, cfg, stride):
        super().__init__()
        self.cfg, self.spatial_scale = cfg, 1.0 / float(stride)
        dim, d = int(cfg.dim_reduced), int(cfg.dilation)
        layers, cin = [], int(dim_in)
        for _ in range(int(cfg.num_convs)):
            layers += [torch.nn.Conv3d(cin, dim, 3, 1, padding=d, dilation=d), torch.nn.ReLU(inplace=True)]
            cin = dim
        self.conv_fcn = torch.nn.Sequential(*layers)
        self.upconv = torch.nn.ConvTranspose3d(dim, dim, 2, 2, 0)
        self.classify = torch.nn.Conv3d(dim, cfg.mask_classes, 1, 1, 0)
        for m in list(self.conv_fcn) + [self.upconv]:
            if not isinstance(m, torch.nn.ReLU):
                torch.nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")     # MRCNN.CONV_INIT: MSRAFill
                torch.nn.init.constant_(m.bias, 0.0)
        if cfg.cls_specific:                                  # mask_rcnn_heads.py:38-46 with CONV_INIT MSRAFill, as both shipped configs set it
            torch.nn.init.kaiming_normal_(self.classify.weight, mode="fan_out", nonlinearity="relu")
        else:
            torch.nn.init.normal_(self.classify.weight, std=0.001)
        torch.nn.init.constant_(self.classify.bias, 0.0)

    def detector_state(self):
        """the parameters under the keys of the reference's detector (and of MaskHeadM3D): Mask_Head.*, Mask_Outs.classify.*"""
        return {("Mask_Outs." if k.startswith("classify") else "Mask_Head.") + k: v for k, v in self.state_dict().items()}

    def load_detector_state(self, params):
        own = {k.split(".", 1)[1]: v for k, v in params.items() if k.startswith(("Mask_Head.", "Mask_Outs."))}
        return self.load_state_dict(own)

    def forward(self, feat, rois7):
        from . import compat
        r = int(self.cfg.roi_xform_resolution)
        x = compat.RoIAlignFunction_3d(r, r, r, self.spatial_scale, int(self.cfg.sampling_ratio))(feat, rois7)
        for m in self.conv_fcn:
            x = compat.conv3d(x, m.weight, m.bias, 1, m.padding, m.dilation) if isinstance(m, torch.nn.Conv3d) else torch.relu(x)
        if compat.get_upconv() == compat.UPCONV_M3D:
            x = upconv3d_2x(x, self.upconv.weight, self.upconv.bias, relu=True)
        else:
            x = torch.relu(self.upconv(x))
        return compat.conv3d(x, self.classify.weight, self.classify.bias, 1, 0)


class ConvBoxHead(torch.nn.Module):
    """roi_Xconv1fc_head followed by fast_rcnn_outputs (fast_rcnn_heads.py:120-179, 12-47) as one module under the reference's parameter
    names convs.{0,2,..}, fc, cls_score, bbox_pred: its state_dict, prefixed Box_Head. / Box_Outs. by `detector_state`, is what
    DetectorM3D takes.  Plain torch modules: under m3d.compat.install() RoIAlign3D, the convolutions and the linear layers run forward and
    backward on the library's kernels (the convs' weight gradient on m3d_conv3d_wgrad, or on the 2 x 8 x 8 tile kernel under
    compat.set_conv_wgrad_narrow(True)); on CPU tensors `trunk` is torch's own arithmetic.  Returns the class scores as logits, as the
    reference does in training."""

    def __init__(self, dim_in, stride, num_classes=2, conv_head_dim=128, num_stacked_convs=2, mlp_head_dim=1024, roi_res=7,
                 sampling_ratio=2, cls_agnostic_bbox_reg=False):
        super().__init__()
        from . import compat
        roi_res, dim = int(roi_res), int(conv_head_dim)
        self.roi_align = compat.RoIAlign_3d(roi_res, roi_res, roi_res, 1.0 / float(stride), int(sampling_ratio))
        layers, cin = [], int(dim_in)
        for _ in range(int(num_stacked_convs)):
            layers += [torch.nn.Conv3d(cin, dim, 3, 1, 1), torch.nn.ReLU(inplace=True)]
            cin = dim
        self.convs = torch.nn.Sequential(*layers)
        self.fc = torch.nn.Linear(cin * roi_res ** 3, int(mlp_head_dim))
        self.cls_score = torch.nn.Linear(int(mlp_head_dim), int(num_classes))
        self.bbox_pred = torch.nn.Linear(int(mlp_head_dim), 6 * (2 if cls_agnostic_bbox_reg else int(num_classes)))
        # The reference's roi_Xconv1fc_head._init_weights (fast_rcnn_heads.py:144-152) tests `isinstance(m, nn.Conv2d)`: its nn.Conv3d layers
        # never match, so they keep torch's default initialisation (kaiming_uniform_(a = sqrt(5)), bias uniform) - MSRAFill is never
        # applied to them.  What it effectively does is kept here: only fc gets XavierFill (uniform +- sqrt(3 / fan_in)) and a zero bias.
        bound = math.sqrt(3.0 / self.fc.in_features)
        torch.nn.init.uniform_(self.fc.weight, -bound, bound)
        torch.nn.init.constant_(self.fc.bias, 0.0)
        torch.nn.init.normal_(self.cls_score.weight, std=0.01)          # fast_rcnn_outputs._init_weights, :23-27
        torch.nn.init.constant_(self.cls_score.bias, 0.0)
        torch.nn.init.normal_(self.bbox_pred.weight, std=0.001)
        torch.nn.init.constant_(self.bbox_pred.bias, 0.0)

    def detector_state(self):
        """the parameters under the keys of the reference's detector (and of DetectorM3D): Box_Head.convs.*, Box_Head.fc.*, Box_Outs.*"""
        return {("Box_Outs." if k.startswith(("cls_score", "bbox_pred")) else "Box_Head.") + k: v for k, v in self.state_dict().items()}

    def load_detector_state(self, params):
        own = {k.split(".", 1)[1]: v for k, v in params.items() if k.startswith(("Box_Head.", "Box_Outs."))}
        return self.load_state_dict(own)

    def trunk(self, pooled):
        """[R, dim_in, r, r, r] RoIAlign output -> (cls_score [R, num_classes] logits, bbox_pred [R, 6 num_classes])"""
        x = self.convs(pooled)
        x = torch.relu(self.fc(x.reshape(x.shape[0], -1)))
        return self.cls_score(x), self.bbox_pred(x)

    def forward(self, feat, rois7):
        return self.trunk(self.roi_align(feat, rois7))
