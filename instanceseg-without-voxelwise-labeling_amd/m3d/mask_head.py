"""Mask branch of the detector: `mask_net` = Mask_Head (RoIAlign3D -> N x [Conv3d 3^3 dilated + ReLU] -> ConvTranspose3d(2, 2) + ReLU)
followed by Mask_Outs (Conv3d 1^3 -> sigmoid), and `im_detect_mask` around it.

Reference: lib/modeling/mask_rcnn_heads.py:132-193 (head), :20-68 (outputs), lib/modeling/model_builder.py:327-331 (mask_net),
lib/core/test.py:439-476 (im_detect_mask).  Both shipped configs run with MODEL.MASK_ON False, so nothing on the headline path
reaches this; it exists so that a MASK_ON checkpoint has somewhere to go.  `segm_results` (core/test.py:886-945) pastes the soft
M^3 masks into the volume on the device (csrc/mask_paste.hip: skimage.transform.resize restated on scipy.ndimage's arithmetic).

Every convolution runs in the HIP library:
  * the dilated 3x3x3 convs through m3d_conv3d_forward_dilated (direct MFMA kernel, halo = dilation); with conv_f16 / M3D_MASK_CONV_F16
    (opt-in) on the narrow-map f16x2 kernel instead (ops.ZnConv3d, csrc/conv3d_zn.hip: dilation 1 and 2, maps at most 8 wide), the
    operand bound carried from conv to conv;
  * ConvTranspose3d(kernel 2, stride 2) never overlaps its outputs, so it is a 1x1x1 conv to 8*Cout channels
    (one per output parity (a,b,c)) followed by a voxel shuffle to the 2x grid; bias + ReLU ride in the conv epilogue.
    Under compat.set_upconv("m3d") it is one m3d_upconv3d_2x_forward instead, whose epilogue writes the 2x grid directly;
  * the 1x1x1 classifier through m3d_conv3d_forward;
  * with tail_f16 / M3D_MASK_TAIL_F16 (opt-in) `mask_net` runs trunk -> ONE launch for up-conv + ReLU + classifier + sigmoid
    (ops.UpConvF16.tail, csrc/upconv3d_f16.hip: the f16x2 cut on the f16 matrix cores); the [R, C, 2M', 2M', 2M'] tensor is never
    written.  `up` and `outputs` stay what they are for callers that use them directly."""
import os

import numpy as np
import torch

from . import conv_plan, ops


class MaskHeadM3D:
    def __init__(self, params, cfg, resolution=None, roi_res=None, sampling_ratio=None, dilation=None, cls_specific=None, conv_f16=None,
                 conv_f16_min_units=None, tail_f16=None, tail_f16_min_rois=None):
        """params: CUDA fp32 tensors under the reference's state-dict keys `Mask_Head.conv_fcn.{0,2,..}.{weight,bias}`,
        `Mask_Head.upconv.{weight,bias}`, `Mask_Outs.classify.{weight,bias}`.  The MRCNN.* settings come from cfg
        (Cfg.from_yaml reads them; defaults = lib/core/config.py:751-780) unless given here.
        conv_f16: the conv_fcn layers on the narrow-map f16x2 kernel (ops.ZnConv3d at the head's dilation, 1 or 2) where it takes the
        layer: cin % 16 == 0, a RoI grid at most 8 wide, and a launch of at least conv_f16_min_units units (None: the measured routing
        threshold of the dilation, conv_plan.ZN_MIN_UNITS / ZN_DILATED_MIN_UNITS; 0 routes every supported launch - tests and A/B runs).
        Every other layer stays on PackedConv3d.  None reads M3D_MASK_CONV_F16 (default "0"); like M3D_HEAD_CONV_F16 it needs
        M3D_CONV_F16 not to be off.  Off, the head is bit for bit what it was without the argument.
        tail_f16: `mask_net` runs the up-conv, its ReLU, the classifier and the sigmoid as one f16x2 launch (ops.UpConvF16.tail) where the
        kernel takes the shape (upconv Cin % 16 == 0, at most 8 mask classes) and the call has at least tail_f16_min_rois RoIs (None:
        conv_plan.MASK_TAIL_F16_MIN_ROIS, the measured threshold; 0 routes every supported call).  The operand bound comes from the last
        trunk conv where that ran on the narrow f16x2 kernel, else from one sweep.  None reads M3D_MASK_TAIL_F16 (default "0"); it needs
        M3D_CONV_F16 not to be off.  Off, the head is bit for bit what it was without the argument."""
        self.cfg = cfg
        resolution = getattr(cfg, "mask_resolution", 14) if resolution is None else resolution
        roi_res = getattr(cfg, "mask_roi_res", 7) if roi_res is None else roi_res
        sampling_ratio = getattr(cfg, "mask_sampling_ratio", 0) if sampling_ratio is None else sampling_ratio
        dilation = getattr(cfg, "mask_dilation", 2) if dilation is None else dilation
        cls_specific = getattr(cfg, "mask_cls_specific", True) if cls_specific is None else cls_specific
        self.M, self.roi_res, self.sampling_ratio, self.dilation = int(resolution), int(roi_res), int(sampling_ratio), int(dilation)
        self.cls_specific = bool(cls_specific)
        if conv_f16 is None:
            conv_f16 = os.environ.get("M3D_MASK_CONV_F16", "0") == "1"
        self.conv_f16 = bool(conv_f16) and os.environ.get("M3D_CONV_F16", "1") == "1" and self.dilation in (1, 2)
        default_units = conv_plan.ZN_DILATED_MIN_UNITS if self.dilation == 2 else conv_plan.ZN_MIN_UNITS
        self.conv_f16_min_units = default_units if conv_f16_min_units is None else int(conv_f16_min_units)
        self.convs, self.zn = [], []                   # zn[i]: the f16x2 pack of conv i, or None (conv_f16 off, or cin % 16 != 0)
        i = 0
        while "Mask_Head.conv_fcn.%d.weight" % (2 * i) in params:                 # mask_rcnn_heads.py:146-153
            w = params["Mask_Head.conv_fcn.%d.weight" % (2 * i)]
            assert tuple(w.shape[2:]) == (3, 3, 3)
            self.convs.append((ops.PackedConv3d(w), params["Mask_Head.conv_fcn.%d.bias" % (2 * i)].contiguous()))
            self.zn.append(ops.ZnConv3d(w) if self.conv_f16 and ops.ZnConv3d.supported(w) else None)
            i += 1
        if not self.convs:
            raise KeyError("no Mask_Head.conv_fcn.* weights in the state dict")
        wu = params["Mask_Head.upconv.weight"]                                      # [Cin, Cout, 2, 2, 2] (:156)
        assert tuple(wu.shape[2:]) == (2, 2, 2)
        cin, cout = int(wu.shape[0]), int(wu.shape[1])
        self.up_cout = cout
        # out[co, 2z+a, 2y+b, 2x+c] = bias[co] + sum_ci in[ci,z,y,x] * W[ci,co,a,b,c]: channel (co,a,b,c) of a 1x1x1 conv
        self.up_pack = ops.PackedConv3d(wu.permute(1, 2, 3, 4, 0).reshape(cout * 8, cin, 1, 1, 1).contiguous())
        self.up_bias = params["Mask_Head.upconv.bias"].repeat_interleave(8).contiguous()
        # compat.set_upconv("m3d"): the weight and bias as stored (csrc/upconv3d.hip reads nn.ConvTranspose3d's layout)
        self.up_weight, self.up_bias_raw = wu.contiguous(), params["Mask_Head.upconv.bias"].contiguous()
        wc = params["Mask_Outs.classify.weight"]                                    # [n_classes or 1, C, 1, 1, 1] (:31)
        assert tuple(wc.shape[2:]) == (1, 1, 1) and wc.shape[0] == (cfg.num_classes if self.cls_specific else 1)
        self.classify = ops.PackedConv3d(wc)
        self.classify_bias = params["Mask_Outs.classify.bias"].contiguous()
        if tail_f16 is None:
            tail_f16 = os.environ.get("M3D_MASK_TAIL_F16", "0") == "1"
        self.tail_f16 = (bool(tail_f16) and os.environ.get("M3D_CONV_F16", "1") == "1" and ops.UpConvF16.supported(wu)
                         and int(wc.shape[0]) <= ops.UpConvF16.MAX_CLASSES)
        self.tail_f16_min_rois = conv_plan.MASK_TAIL_F16_MIN_ROIS if tail_f16_min_rois is None else int(tail_f16_min_rois)
        self.up_f16 = ops.UpConvF16(wu) if self.tail_f16 else None
        self.classify_weight = wc.reshape(int(wc.shape[0]), cout).contiguous() if self.tail_f16 else None
        self._ones = {}

    def _one(self, n, device):
        t = self._ones.get(n)
        if t is None:
            t = self._ones[n] = torch.ones((n,), dtype=torch.float32, device=device)
        return t

    def _zn_takes(self, i, shape):
        """conv i runs on the f16x2 kernel for an input of this shape [R, cin, M', M', M']"""
        zn = self.zn[i]
        return (zn is not None and shape[0] > 0 and zn.supports(shape, dilation=self.dilation)
                and zn.units(shape, dilation=self.dilation) >= self.conv_f16_min_units)

    def _tail_takes(self, shape):
        """`mask_net` runs the fused tail on a trunk output of this shape [R, C, M', M', M']"""
        return (self.tail_f16 and shape[0] > 0 and shape[0] >= self.tail_f16_min_rois and self.up_f16.supports(shape))

    def trunk(self, feat, mask_rois, feat_max=None, want_bound=False):
        """RoIAlign3D and the dilated convs of Mask_Head.forward (mask_rcnn_heads.py:181-192): [R, C, M', M', M'] with M' = roi_res.
        feat_max (conv_f16 only): the operand bound of feat as the conv that produced it left it ([ZwConv3d.SLOTS] device floats, the
        largest = a bound of max |feat|).  Every RoIAlign value is a convex combination of feature-map values, so it bounds the first
        conv's input too (the argument DetectorM3D uses for the conv box head); None: one ZwConv3d.bound_of sweep of the RoIAlign
        output.  Each conv's epilogue leaves the next conv's bound.
        want_bound: -> (x, bound): the last conv, where it runs on the f16x2 kernel, leaves the bound of its output for the fused tail
        (None where it ran on the fp32 kernel).  Without it the last conv is asked for no bound, as before."""
        c = self.cfg
        x = ops.roi_align3d_forward(feat, mask_rois, self.roi_res, self.roi_res, self.roi_res, 1.0 / c.stride, self.sampling_ratio)
        bound = feat_max                               # the bound of x where one is held, else None
        last = len(self.convs) - 1
        for i, (conv, bias) in enumerate(self.convs):
            if self.conv_f16 and self._zn_takes(i, tuple(x.shape)):
                if bound is None:
                    bound = ops.ZwConv3d.bound_of(x)
                nxt = i < last and self._zn_takes(i + 1, (x.shape[0], conv.cout) + tuple(x.shape[2:]))
                nxt = nxt or (want_bound and i == last)
                x, bound = self.zn[i](x, bound, shift=bias, relu=True, out_max=None if nxt else False, dilation=self.dilation)
            else:
                x = conv(x, scale=self._one(conv.cout, x.device), shift=bias, relu=True, dilation=self.dilation)
                bound = None
        return (x, bound) if want_bound else x

    def up(self, x):
        """upconv + ReLU (mask_rcnn_heads.py:193): [R, C, M', M', M'] -> [R, Cout, 2M', 2M', 2M'].  compat.set_upconv("m3d"): one
        m3d_upconv3d_2x_forward on the weight as stored; "torch" (the default): the 1x1x1 conv to 8 Cout channels + voxel shuffle."""
        from . import compat
        if compat.get_upconv() == compat.UPCONV_M3D:
            return ops.upconv3d_2x_forward(x, self.up_weight, self.up_bias_raw, relu=True)
        y = self.up_pack(x, scale=self._one(self.up_pack.cout, x.device), shift=self.up_bias, relu=True)   # ReLU is pointwise
        R, d, h, w = y.shape[0], x.shape[2], x.shape[3], x.shape[4]
        y = y.view(R, self.up_cout, 2, 2, 2, d, h, w).permute(0, 1, 5, 2, 6, 3, 7, 4)
        return y.reshape(R, self.up_cout, 2 * d, 2 * h, 2 * w)

    def head(self, feat, mask_rois):
        """Mask_Head.forward (mask_rcnn_heads.py:181-193): [R, C, 2M', 2M', 2M'] with M' = roi_res."""
        return self.up(self.trunk(feat, mask_rois))

    def outputs(self, x):
        """Mask_Outs.forward in eval mode (mask_rcnn_heads.py:62-68, UPSAMPLE_RATIO 1, USE_FC_OUTPUT False)."""
        y = self.classify(x, scale=self._one(self.classify.cout, x.device), shift=self.classify_bias)
        return torch.sigmoid(y)

    def mask_net(self, blob_conv, rpn_blob):
        """model_builder.py:327-331: rpn_blob = {'mask_rois': [R, 7] (batch, x1, y1, z1, x2, y2, z2)} (tensor or ndarray)."""
        rois = rpn_blob["mask_rois"] if isinstance(rpn_blob, dict) else rpn_blob
        if not torch.is_tensor(rois):
            rois = torch.from_numpy(np.ascontiguousarray(rois, dtype=np.float32))
        rois = rois.to(device=blob_conv.device, dtype=torch.float32)
        if self.tail_f16 and self._tail_takes((int(rois.shape[0]), self.up_f16.cin) + (self.roi_res,) * 3):
            x, bound = self.trunk(blob_conv, rois, want_bound=True)
            return self.up_f16.tail(x, bound, self.up_bias_raw, self.classify_weight, self.classify_bias, sigmoid=True)
        return self.outputs(self.head(blob_conv, rois))


def im_detect_mask(mask_head, im_scale, boxes, blob_conv):
    """lib/core/test.py:439-476.  boxes: ndarray [R, 6] in image coordinates; returns ndarray [R, K, M, M, M] float32
    (K = NUM_CLASSES when class specific, else 1); [0, M, M, M] for no boxes (:457-459)."""
    M = mask_head.M
    boxes = np.asarray(boxes)
    if boxes.shape[0] == 0:
        return np.zeros((0, M, M, M), np.float32)
    scale = float(im_scale[0] if np.ndim(im_scale) else im_scale)
    rois = np.hstack([np.zeros((boxes.shape[0], 1)), boxes.astype(np.float64) * scale]).astype(np.float32)   # _get_rois_blob (:967-980)
    pred = mask_head.mask_net(blob_conv, {"mask_rois": rois})
    pred = pred.cpu().numpy().squeeze()                                                                       # :469
    K = mask_head.cfg.num_classes if mask_head.cls_specific else 1
    return pred.reshape([-1, K, M, M, M])                                                                     # :471-474


def expand_boxes(boxes, scale):
    """lib/utils/boxes_3d.py:271-292."""
    boxes = np.asarray(boxes, dtype=np.float64)
    half = (boxes[:, 3:6] - boxes[:, 0:3]) * .5 * scale
    ctr = (boxes[:, 3:6] + boxes[:, 0:3]) * .5
    return np.hstack([ctr - half, ctr + half])


def segm_results(cls_boxes, masks, ref_boxes, im_s, im_h, im_w, num_classes=2, resolution=None, cls_specific=True, thresh=0.5,
                 device="cuda"):
    """lib/core/test.py:886-945 with the reference's signature (the cfg values are keyword arguments): cls_boxes = per-class lists
    of [n_j, 7] detections, masks [R, K, M, M, M] from im_detect_mask, ref_boxes [R, 6] (the same class-major order).
    Returns cls_segms: per class a list of [im_s, im_h, im_w] uint8 arrays (host, as the reference)."""
    masks_t = masks if torch.is_tensor(masks) else torch.from_numpy(np.ascontiguousarray(masks, dtype=np.float32))
    masks_t = masks_t.to(device)
    M = int(masks_t.shape[-1]) if resolution is None else int(resolution)
    rb = expand_boxes(ref_boxes, (M + 2.0) / M).astype(np.int32)                              # :896-898
    counts = [0] + [int(cls_boxes[j].shape[0]) for j in range(1, num_classes)]
    assert sum(counts) == masks_t.shape[0], "segm_results: masks and cls_boxes disagree"        # :944
    channel = np.concatenate([np.full((counts[j],), j if cls_specific else 0, np.int32) for j in range(num_classes)]) \
        if masks_t.shape[0] else np.zeros((0,), np.int32)
    pasted = ops.mask_paste3d(masks_t, channel, rb, (im_s, im_h, im_w), thresh).cpu().numpy()
    cls_segms, ind = [[] for _ in range(num_classes)], 0
    for j in range(1, num_classes):
        cls_segms[j] = [pasted[ind + i] for i in range(counts[j])]
        ind += counts[j]
    return cls_segms
