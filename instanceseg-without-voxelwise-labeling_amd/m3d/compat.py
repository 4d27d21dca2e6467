"""Drop-in modules under the reference's own dotted names, backed by libm3d.so.

    import m3d.compat; m3d.compat.install()          # before `import modeling...` / `import utils...`

registers:
  modeling.roi_xfrom.roi_align_3d.functions.roi_align_3d   RoIAlignFunction_3d          (functions/roi_align_3d.py:7-51)
  modeling.roi_xfrom.roi_align_3d.modules.roi_align_3d     RoIAlign_3d / Avg_3d / Max_3d (modules/roi_align_3d.py:6-48)
  utils.cython_nms_3d      nms_3d, nms_3d_volume, soft_nms_3d                            (lib/utils/cython_nms_3d.pyx)
  utils.cython_bbox_3d     bbox_overlaps_3d                                              (lib/utils/cython_bbox_3d.pyx)
  model.roi_pooling.functions.roi_pool / model.roi_crop.functions.roi_crop   import-compat shims (2D legacy,
                           model_builder.py:11-12 imports them; the 3D path never calls them)
  otsu                     otsu_py_2d_fast                                               (tools/otsu.py:199-284)
and install_conv3d() routes qualifying torch.nn.functional.conv3d calls (fp32, CUDA, NCDHW, stride 1,
padding k//2, dilation 1, groups 1, k in {1,3} or the 5^3/Cin=1 stem) to the MFMA kernels, forward and
backward-data, so lib/modeling/DSN.py and lib/prm/peak_backprop_3d.py run unchanged on them.  Under set_conv_dilated("m3d")
(opt-in) the k = 3, dilation 2, padding 2 convs of the mask head go there too, forward and backward.  Under
set_conv_wgrad_narrow(True) (opt-in) the weight gradient of the dilation-1 3^3 convs on maps at most 8 wide - the per-RoI convs of the
conv box head and of the mask head - runs on the 2 x 8 x 8 tile kernel (m3d_conv3d_wgrad_narrow).
set_conv_wgrad_narrow_f16(True) (opt-in) runs that weight gradient on the f16 matrix cores instead (m3d_conv3d_wgrad_narrow_f16x2).
set_conv_dilated_f16(True) (opt-in, under set_conv_dilated("m3d")) runs the forward and the backward-data pass of the dilation-2 convs on
maps at most 8 wide on the dilation-2 instantiation of the narrow-map f16x2 kernel (m3d_conv3d_zn_dilated_forward).
set_conv_train_narrow(True) (opt-in) runs the forward and the backward-data pass of those same convs on the narrow-map f16x2 kernel
(m3d_conv3d_zn_forward, csrc/conv3d_zn.hip).
What the setters say is one conv_plan.TrainSetting; what a routed conv launches under it, forward and backward, is decided by
conv_plan.plan_train_conv alone, and the one conv Function (_Conv3dFn) runs that plan.
"""
import importlib
import sys
import types
import weakref

import numpy as np
import torch

from . import conv_plan, ops


# ----------------------------------------------------------------------------- RoIAlign3D
ROI_BACKWARD_ATOMIC, ROI_BACKWARD_ORDERED = "atomic", "ordered"
_roi_align_backward = ROI_BACKWARD_ATOMIC


def set_roi_align_backward(mode):
    """The backward kernel of the RoIAlign Function (RoIAlign_3d / RoIAlignAvg_3d / RoIAlignMax_3d / RoIAlignFunction_3d): "atomic" (the
    default; install() does not change it) keeps m3d_roi_align3d_backward, whose fp32 atomic adds meet in an order nobody chooses;
    "ordered" takes m3d_roi_align3d_backward_ordered (no atomics, bit-identical from run to run; DESIGN, "RoIAlign3D backward, ordered").
    The forward is the same under both.  In "ordered" mode a configuration that kernel does not take (an adaptive grid beyond the tables)
    raises M3DError; it does not fall back.  Returns the previous mode."""
    global _roi_align_backward
    if mode not in (ROI_BACKWARD_ATOMIC, ROI_BACKWARD_ORDERED):
        raise ValueError("set_roi_align_backward(%r): 'atomic' or 'ordered'" % (mode,))
    prev, _roi_align_backward = _roi_align_backward, mode
    return prev


def get_roi_align_backward():
    return _roi_align_backward


class _RoIAlign3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, rois, AS, AH, AW, scale, ratio):
        ctx.save_for_backward(rois)
        ctx.cfg = (AS, AH, AW, scale, ratio, tuple(features.shape))
        return ops.roi_align3d_forward(features, rois, AS, AH, AW, scale, ratio)

    @staticmethod
    def backward(ctx, grad_output):
        rois, = ctx.saved_tensors
        AS, AH, AW, scale, ratio, fshape = ctx.cfg
        fn = ops.roi_align3d_backward_ordered if _roi_align_backward == ROI_BACKWARD_ORDERED else ops.roi_align3d_backward
        g = fn(grad_output.contiguous(), rois, fshape, AS, AH, AW, scale, ratio)
        return g, None, None, None, None, None, None


class RoIAlignFunction_3d(object):
    """Same call shape as the reference's legacy instance-style Function:
    RoIAlignFunction_3d(AS, AH, AW, scale, ratio)(features, rois)   (model_builder.py:311-312)."""

    def __init__(self, aligned_slices, aligned_height, aligned_width, spatial_scale, sampling_ratio):
        self.aligned_slices = int(aligned_slices)
        self.aligned_width = int(aligned_width)
        self.aligned_height = int(aligned_height)
        self.spatial_scale = float(spatial_scale)
        self.sampling_ratio = int(sampling_ratio)

    def __call__(self, features, rois):
        if not features.is_cuda:
            raise NotImplementedError          # functions/roi_align_3d.py:31-32
        return _RoIAlign3dFn.apply(features, rois, self.aligned_slices, self.aligned_height, self.aligned_width,
                                   self.spatial_scale, self.sampling_ratio)


class RoIAlign_3d(torch.nn.Module):
    def __init__(self, aligned_slices, aligned_height, aligned_width, spatial_scale, sampling_ratio):
        super().__init__()
        self.aligned_width, self.aligned_height, self.aligned_slices = int(aligned_width), int(aligned_height), int(aligned_slices)
        self.spatial_scale, self.sampling_ratio = float(spatial_scale), int(sampling_ratio)

    def _fn(self, extra):
        return RoIAlignFunction_3d(self.aligned_slices + extra, self.aligned_height + extra, self.aligned_width + extra,
                                   self.spatial_scale, self.sampling_ratio)

    def forward(self, features, rois):
        return self._fn(0)(features, rois)


class RoIAlignAvg_3d(RoIAlign_3d):
    def forward(self, features, rois):       # modules/roi_align_3d.py:30-33
        return torch.nn.functional.avg_pool3d(self._fn(1)(features, rois), kernel_size=2, stride=1)


class RoIAlignMax_3d(RoIAlign_3d):
    def forward(self, features, rois):       # modules/roi_align_3d.py:45-48
        return torch.nn.functional.max_pool3d(self._fn(1)(features, rois), kernel_size=2, stride=1)


# ----------------------------------------------------------------------------- Cython-API box ops (NumPy in/out)
def _check_f32_2d(a, name):
    # Cython buffer typing `np.ndarray[np.float32_t, ndim=2]` rejects anything else with ValueError
    if not isinstance(a, np.ndarray):
        raise TypeError("Argument '%s' has incorrect type (expected numpy.ndarray, got %s)" % (name, type(a).__name__))
    if a.ndim != 2:
        raise ValueError("Buffer has wrong number of dimensions (expected 2, got %d)" % a.ndim)
    if a.dtype != np.float32:
        raise ValueError("Buffer dtype mismatch, expected 'float32_t' but got '%s'" % a.dtype)


def nms_3d(dets, thresh):
    _check_f32_2d(dets, "dets")
    d = torch.from_numpy(np.ascontiguousarray(dets)).cuda()
    return ops.nms3d(d, thresh).cpu().numpy()


def nms_3d_volume(dets, thresh):
    _check_f32_2d(dets, "dets")
    d = torch.from_numpy(np.ascontiguousarray(dets)).cuda()
    return ops.nms3d(d, thresh, by_volume=True).cpu().numpy()


def soft_nms_3d(boxes_in, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    raise NotImplementedError(
        "soft_nms_3d is unreachable in the reference (TEST.SOFT_NMS.ENABLED=False, core/config.py:370; the wrapper "
        "boxes_3d.soft_nms is mis-named vs its caller core/test.py:843 and the kernel overwrites column 4 three times, "
        "cython_nms_3d.pyx:280-282); deliberately not reproduced")


def bbox_overlaps_3d(boxes, query_boxes):
    _check_f32_2d(boxes, "boxes")
    _check_f32_2d(query_boxes, "query_boxes")
    b = torch.from_numpy(np.ascontiguousarray(boxes)).cuda()
    q = torch.from_numpy(np.ascontiguousarray(query_boxes)).cuda()
    return ops.bbox_overlaps3d(b, q).cpu().numpy()


def otsu_py_2d_fast(image, prm, b_range=None):
    """tools/otsu.py:199 signature; uint16 volumes (what both callers pass).  Returns (uint8 mask, k, b)."""
    if b_range is not None:
        raise NotImplementedError("b_range is never passed by the reference callers")
    img = np.ascontiguousarray(image)
    pr = np.ascontiguousarray(prm)
    if img.dtype != np.uint16 or pr.dtype != np.uint16:
        raise TypeError("otsu_py_2d_fast (HIP) takes the uint16 crops the reference callers produce")
    offs = torch.tensor([0, img.size], dtype=torch.int64, device="cuda")
    G = int(img.max()) - int(img.min()) + 1
    mask, kb, status = ops.otsu2d_batch(torch.from_numpy(img.ravel()).cuda(), torch.from_numpy(pr.ravel()).cuda(), offs,
                                        max_gray_range=max(G, 2))
    if int(status[0]) != 0:
        raise UnboundLocalError("local variable 'k_max' referenced before assignment")   # otsu.py:277 behaviour
    return mask.cpu().numpy().reshape(img.shape), int(kb[0, 0]), int(kb[0, 1])


class _Legacy2D(object):
    def __init__(self, *a, **k):
        raise NotImplementedError("2D legacy op: no 3D version exists in the reference (SURVEY 8a-15)")


# ----------------------------------------------------------------------------- F.conv3d interception
_orig_conv3d = None
_pack_cache = {}          # (id(parameter), pack kind) -> (weakref to the parameter, _version, data_ptr, pack)


def _stem_dgrad_pack(weight):
    """the backward-data of the 5^3 / Cin = 1 stem as a pack that is called on gy, like the others: its tap-flipped [C,125] weights"""
    wf = ops.conv3d_stem5_dgrad_weights(weight)
    return lambda gy: ops.conv3d_stem5_dgrad(gy, wf)


_PACKS = {                # pack kind -> constructor from the detached weight
    "plain": lambda w: ops.PackedConv3d(w, ops.W_PLAIN),     # the direct fp32 kernel, forward (dilation 1 and 2)
    "dgrad": lambda w: ops.PackedConv3d(w, ops.W_DGRAD),     # ... its backward-data
    "stem-dgrad": _stem_dgrad_pack,
    "zw-plain": ops.ZwConv3d, "zw-dgrad": ops.ZwConv3d.dgrad_of,       # the f16x2 kernel (set_conv_train)
    "zn-plain": ops.ZnConv3d, "zn-dgrad": ops.ZnConv3d.dgrad_of,       # the narrow-map f16x2 kernel (set_conv_train_narrow)
    "upconv-f16": ops.UpConvF16,                             # the up-conv's f16x2 forward (set_upconv_f16)
}


def _packed(weight, mode):
    """MFMA-order pack of `weight`.  Only nn.Parameters are cached, and a cached pack is served only to the SAME live
    object at the same `_version` and address: the reference's pr_conv3d passes a fresh `F.relu(self.weight).detach()`
    every call (peak_backprop_3d.py:41) whose address the allocator may later hand to another layer's temporary of the
    same shape - temporaries are therefore re-packed on every call (7-25 us, small next to the conv)."""
    if not isinstance(weight, torch.nn.Parameter):
        return _PACKS[mode](weight.detach())
    key = (id(weight), mode)
    ent = _pack_cache.get(key)
    if ent is not None:
        ref, ver, ptr, pack = ent
        if ref() is weight and ver == weight._version and ptr == weight.data_ptr():
            return pack
    pack = _PACKS[mode](weight.detach())
    _pack_cache[key] = (weakref.ref(weight, lambda _r, k=key: _pack_cache.pop(k, None)), weight._version, weight.data_ptr(), pack)
    return pack


_setting = conv_plan.TrainSetting()          # everything the setters below say; WHEN each field is read: the TrainSetting docstring


def _threshold(setter, name, value):
    """a routing threshold as a setter takes it: None (the setter's default) or a count >= 0"""
    if value is not None and int(value) < 0:
        raise ValueError("%s(%s=%r): None or a count >= 0" % (setter, name, value))
    return None if value is None else int(value)


def _set_mode(field, modes, mode, **thresholds):
    """set_conv_<field>(mode, **thresholds): one mode string out of the two `modes` into _setting.<field>, each threshold (checked after
    the mode) into the field of its name -> the previous mode"""
    global _setting
    if mode not in modes:
        raise ValueError("set_conv_%s(%r): %r or %r" % ((field, mode) + tuple(modes)))
    also = {name: _threshold("set_conv_" + field, name, value) for name, value in thresholds.items()}
    prev, _setting = getattr(_setting, field), _setting._replace(**{field: mode}, **also)
    return prev


def _set_switch(setter, field, on, name, value, default):
    """setter(on, name=value): an on / off switch with a routing threshold, kept in _setting.<field> as None (off) or the threshold
    (value None: `default`) -> whether it was on"""
    global _setting
    value = _threshold(setter, name, value)
    prev, _setting = getattr(_setting, field) is not None, _setting._replace(**{field: (default if value is None else value) if on else None})
    return prev


def set_conv_wgrad(mode):
    """The weight-gradient kernel of the intercepted convs: "fp32" (the default; install() does not change it) keeps m3d_conv3d_wgrad;
    "f16x2" takes m3d_conv3d_wgrad_f16x2 (the f16 matrix cores at fp32 accuracy, two operand sweeps included) for the layers
    conv_plan.wgrad_kernel routes to it - every other layer (the 5^3 stem, k = 1, channel counts that are no multiple of 32) stays on the
    fp32 kernel.  Forward, dgrad and the bias gradient are the same under both settings.  Returns the previous setting."""
    return _set_mode("wgrad", (conv_plan.WGRAD_FP32, conv_plan.WGRAD_F16X2), mode)


def get_conv_wgrad():
    return _setting.wgrad


def set_conv_wgrad_narrow(on):
    """The dilation-1 weight gradient of the intercepted 3^3 convs on maps at most 8 wide (the per-RoI convs of train.ConvBoxHead and of
    train.MaskHead at dilation 1, on 7^3 grids): False (the default; install() does not change it) keeps m3d_conv3d_wgrad, whose
    2 x 4 x 16 voxel tile such a map fills to a third; True takes m3d_conv3d_wgrad_narrow (2 x 8 x 8) for the layers
    conv_plan.wgrad_kernel(narrow=True) routes to it.  A layer that set_conv_wgrad("f16x2") routes to the f16 kernel stays there; the
    forward, dgrad and the bias gradient are the same under both settings.  Returns the previous setting."""
    global _setting
    prev, _setting = _setting.wgrad_narrow, _setting._replace(wgrad_narrow=bool(on))
    return prev


def get_conv_wgrad_narrow():
    return _setting.wgrad_narrow


def set_conv_wgrad_narrow_f16(on, min_work=None):
    """The weight gradient of the intercepted 3^3 convs on maps at most 8 wide with channel counts that are multiples of 32 (the per-RoI
    convs on 7^3 grids): False (the default; install() does not change it) keeps what set_conv_wgrad and set_conv_wgrad_narrow give
    them; True takes m3d_conv3d_wgrad_narrow_f16x2 (the f16 matrix cores at fp32 accuracy on the 2 x 8 x 8 tile) for the layers
    conv_plan.wgrad_kernel(narrow_f16=) routes to it, whatever those two switches say.  x's bound comes from the forward and gy's from
    m3d_conv3d_gy_reduce where set_conv_train_narrow / set_conv_train ran them, else the kernel's wrapper sweeps; forward, dgrad and the
    bias gradient are the same with the switch on or off.  min_work: the routing threshold in products per tap, batch D H W cin cout
    (None: conv_plan.WGRAD_NARROW_F16X2_MIN_WORK; 0 routes every supported layer - tests and A/B runs; a call without it puts the
    default back).  Read when the backward runs.  Returns the previous setting (True / False)."""
    return _set_switch("set_conv_wgrad_narrow_f16", "wgrad_narrow_f16", on, "min_work", min_work, conv_plan.WGRAD_NARROW_F16X2_MIN_WORK)


def get_conv_wgrad_narrow_f16():
    return _setting.wgrad_narrow_f16 is not None


def set_conv_train(mode, min_units=None):
    """The forward and backward-data kernels of the intercepted convs: "fp32" (the default; install() does not change it) keeps the direct
    fp32 MFMA kernel for both; "f16x2" takes m3d_conv3d_zw_forward (the f16 matrix cores at fp32 accuracy, Winograd F(2,3) along z) for the
    layers and directions conv_plan.train_conv_kernel routes to it - every other layer (the 5^3 stem, k = 1, input channels that are no
    multiple of 16, small maps, fewer than 32 output channels) stays on the fp32 kernel.  In mode "f16x2" the bias gradient of
    every layer comes from m3d_conv3d_gy_reduce (fp64 sums, one rounding), whichever kernels the layer routes to, and that one pass over gy
    also gives the operand bound the f16x2 dgrad and the f16x2 wgrad (set_conv_wgrad) share; the forward sweeps x once and keeps the bound
    for the wgrad.  min_units: the routing threshold in launch units (None: conv_plan.ZW_MIN_UNITS; 0 routes every supported layer - tests
    and A/B runs; a call without it puts the default back).  Returns the previous mode.
    As set_conv_wgrad("f16x2") already implies for its kernel: with a non-finite value in an operand the operand's bound is non-finite and
    the WHOLE result is, not only the elements the fp32 kernel's element-wise propagation would reach; Solver(stats=True).nonfinite is
    the guard."""
    return _set_mode("train", (conv_plan.TRAIN_FP32, conv_plan.TRAIN_F16X2), mode, min_units=min_units)


def get_conv_train():
    return _setting.train


def set_conv_train_narrow(on, min_units=None):
    """The forward and backward-data kernels of the intercepted 3^3 convs on maps at most 8 wide (the per-RoI convs of train.ConvBoxHead
    and of train.MaskHead at dilation 1, on 7^3 grids): False (the default; install() does not change it) keeps what set_conv_train
    gives them - the direct fp32 MFMA kernel, the zw kernel takes no map narrower than 12; True takes the narrow-map f16x2 kernel
    (ops.ZnConv3d, csrc/conv3d_zn.hip; dgrad on its dgrad_of pack) for the layers and directions
    conv_plan.train_conv_kernel(narrow=True) routes to it.  Such a forward sweeps x once; such a dgrad takes gy's bound from
    m3d_conv3d_gy_reduce, which then also gives the bias gradient (as set_conv_train("f16x2") does).  Independent of set_conv_train; the
    weight gradient's routing (set_conv_wgrad, set_conv_wgrad_narrow) is untouched.  min_units: the routing threshold in launch units
    (None: conv_plan.ZN_MIN_UNITS; 0 routes every supported layer - tests and A/B runs; a call without it puts the default back).
    Returns the previous setting (True / False)."""
    return _set_switch("set_conv_train_narrow", "narrow", on, "min_units", min_units, conv_plan.ZN_MIN_UNITS)


def get_conv_train_narrow():
    return _setting.narrow is not None


CONV_DILATED_TORCH, CONV_DILATED_M3D = conv_plan.DILATED_TORCH, conv_plan.DILATED_M3D


def set_conv_dilated(mode):
    """The 3^3 convs with dilation 2 and padding 2 (the mask head at MRCNN.DILATION = 2, train.MaskHead): "torch" (the default;
    install() does not change it) leaves them to torch's own conv3d, as every other dilation always is; "m3d" takes the library in
    training: forward m3d_conv3d_forward_dilated, gx the same on the W_DGRAD pack, gw m3d_conv3d_wgrad_dilated, gb m3d_conv3d_bias_grad
    (DESIGN, "Dilated conv backward").  All fp32: set_conv_train("f16x2") and set_conv_wgrad("f16x2") do not reach these layers;
    set_conv_dilated_f16 (opt-in) moves their forward and dgrad on narrow maps to the f16 matrix cores.  The backward of a call follows
    the mode its forward ran under.  Returns the previous mode."""
    return _set_mode("dilated", (CONV_DILATED_TORCH, CONV_DILATED_M3D), mode)


def get_conv_dilated():
    return _setting.dilated


def set_conv_dilated_f16(on, min_units=None):
    """The forward and backward-data kernels of the dilation-2 convs that set_conv_dilated("m3d") routes to the library, on maps at most
    8 wide with launched input channels a multiple of 16 (train.MaskHead at MRCNN.DILATION = 2 on 7^3 RoI grids): False (the default;
    install() does not change it) keeps m3d_conv3d_forward_dilated, the direct fp32 kernel; True takes the dilation-2 instantiation of
    the narrow-map f16x2 kernel (ops.ZnConv3d(..., dilation=2), csrc/conv3d_zn.hip; dgrad on its dgrad_of pack) for the layers and
    directions conv_plan.plan_train_conv routes to it (TrainSetting.dilated_f16).  Such a forward sweeps x once; such a dgrad takes gy's bound from
    m3d_conv3d_gy_reduce, which then also gives the bias gradient (the rule of set_conv_train_narrow).  The weight gradient stays on
    m3d_conv3d_wgrad_dilated.  Without set_conv_dilated("m3d") it has no effect.  min_units: the routing threshold in launch units
    (None: conv_plan.ZN_DILATED_MIN_UNITS; 0 routes every supported layer - tests and A/B runs; a call without it puts the default
    back).  Read at forward time; the backward of a call follows the value its forward ran under.  Returns the previous setting
    (True / False)."""
    return _set_switch("set_conv_dilated_f16", "dilated_f16", on, "min_units", min_units, conv_plan.ZN_DILATED_MIN_UNITS)


def get_conv_dilated_f16():
    return _setting.dilated_f16 is not None


def set_conv_wgrad_dilated_f16(on, min_work=None):
    """The weight gradient of the dilation-2 convs that set_conv_dilated("m3d") routes to the library, on maps at most 8 wide with channel
    counts that are multiples of 32 (train.MaskHead at MRCNN.DILATION = 2 on 7^3 RoI grids): False (the default; install() does not
    change it) keeps m3d_conv3d_wgrad_dilated, the fp32 kernel; True takes m3d_conv3d_wgrad_narrow_dilated_f16x2 (the f16 matrix cores
    at fp32 accuracy on the 2 x 8 x 8 tile, dilation 2) for the layers conv_plan.plan_train_conv routes to it (TrainSetting.wgrad_dilated_f16).  x's
    bound comes from the forward and gy's from m3d_conv3d_gy_reduce where set_conv_dilated_f16 ran them, else the kernel's wrapper
    sweeps; forward, dgrad and the bias gradient are the same with the switch on or off.  Without set_conv_dilated("m3d") it has no
    effect.  min_work: the routing threshold in products per tap, batch D H W cin cout (None:
    conv_plan.WGRAD_DILATED_F16X2_MIN_WORK; 0 routes every supported layer - tests and A/B runs; a call without it puts the default
    back).  Read when the backward runs.  Returns the previous setting (True / False)."""
    return _set_switch("set_conv_wgrad_dilated_f16", "wgrad_dilated_f16", on, "min_work", min_work, conv_plan.WGRAD_DILATED_F16X2_MIN_WORK)


def get_conv_wgrad_dilated_f16():
    return _setting.wgrad_dilated_f16 is not None


# forward / dgrad kind of the plan -> (pack family: "plain" or "dgrad" follows by direction; dilation; the call takes an operand bound)
_CONV_KINDS = {
    conv_plan.TRAIN_FP32: ("", 1, False),
    conv_plan.TRAIN_F16X2: ("zw-", 1, True),
    conv_plan.TRAIN_F16X2_NARROW: ("zn-", 1, True),
    conv_plan.TRAIN_DILATED: ("", 2, False),
    conv_plan.TRAIN_DILATED_F16X2: ("zn-", 2, True),
    conv_plan.DGRAD_STEM: ("stem-", 1, False),
}
# wgrad kind of the plan -> its call on (x, gy, x's bound, gy's bound, k).  The f16x2 kernels take x's bound from the forward where that
# ran on an f16x2 kernel and gy's from the reduce where that ran; a missing one is swept.  The narrow f16x2 kernel is one wrapper at
# either dilation (1: it makes the calls it made before it had the keyword)
_WGRAD_KINDS = {
    conv_plan.WGRAD_FP32: lambda x, gy, x_max, gy_max, k: ops.conv3d_wgrad(x, gy, k),
    conv_plan.WGRAD_F16X2: lambda x, gy, x_max, gy_max, k: ops.conv3d_wgrad_f16x2(x, gy, x_max, gy_max),
    conv_plan.WGRAD_NARROW: lambda x, gy, x_max, gy_max, k: ops.conv3d_wgrad_narrow(x, gy),
    conv_plan.WGRAD_NARROW_F16X2: lambda x, gy, x_max, gy_max, k: ops.conv3d_wgrad_narrow_f16x2(x, gy, x_max, gy_max, dilation=1),
    conv_plan.WGRAD_DILATED: lambda x, gy, x_max, gy_max, k: ops.conv3d_wgrad(x, gy, 3, dilation=2),
    conv_plan.WGRAD_DILATED_F16X2: lambda x, gy, x_max, gy_max, k: ops.conv3d_wgrad_narrow_f16x2(x, gy, x_max, gy_max, dilation=2),
}


def _run_conv(kind, weight, direction, x, bound, **kw):
    """the conv of plan kind `kind` (a key of _CONV_KINDS; an unknown one is a KeyError) on x: the forward (direction "plain"; kw: shift)
    or the backward-data pass (direction "dgrad", x is gy)"""
    family, dilation, bounded = _CONV_KINDS[kind]
    if dilation != 1:
        kw["dilation"] = dilation
    pack = _packed(weight, family + direction)
    return pack(x, bound, out_max=False, **kw)[0] if bounded else pack(x, **kw)


class _Conv3dFn(torch.autograd.Function):
    """A conv that conv3d() routes to the library (dilation 1 or 2): runs conv_plan.plan_train_conv's plan, the forward half in
    forward, the backward half in backward, from the two tables above.  Nothing is decided here."""

    @staticmethod
    def forward(ctx, x, weight, bias, dilation):
        ctx.save_for_backward(weight, x if weight.requires_grad else None)
        ctx.has_bias = bias is not None
        ctx.setting, ctx.xshape, ctx.dilation = _setting, tuple(x.shape), dilation      # (when each field is read: TrainSetting)
        shift = bias.detach().contiguous() if bias is not None else None
        kind, sweep = conv_plan.plan_train_forward(ctx.setting, ctx.xshape, weight.shape, dilation)
        ctx.x_max = ops.ZwConv3d.bound_of(x) if sweep else None        # kept for the f16x2 wgrad
        return _run_conv(kind, weight, "plain", x, ctx.x_max, shift=shift)

    @staticmethod
    def backward(ctx, gy):
        weight, x = ctx.saved_tensors
        gy = gy.contiguous()
        setting = ctx.setting._replace(**{field: getattr(_setting, field) for field in conv_plan.BACKWARD_FIELDS})
        needs = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        dgrad, wgrad, gy_reduce, gb_from = conv_plan.plan_train_backward(setting, ctx.xshape, weight.shape, ctx.dilation, needs)
        gb = gy_max = None
        if gy_reduce:
            gb, gy_max = ops.conv3d_gy_reduce(gy, bias=gb_from == conv_plan.GB_REDUCE)
        gx = None if dgrad is None else _run_conv(dgrad, weight, "dgrad", gy, gy_max)
        gw = None if wgrad is None else _WGRAD_KINDS[wgrad](x, gy, ctx.x_max, gy_max, weight.shape[2])
        if gb_from == conv_plan.GB_BIAS_GRAD:
            gb = ops.conv3d_bias_grad(gy)
        return gx, gw, gb, None


def _routed_dilation(x, weight, bias, stride, padding, dilation, groups):
    """The dilation of the library conv this call runs as, or None for torch's own.  1: fp32, CUDA, NCDHW, stride 1, padding k // 2,
    groups 1, k in {1, 3} or the 5^3 / Cin = 1 stem (any strides of x: the caller makes it contiguous; nothing is asked of the bias).
    2, only under set_conv_dilated("m3d"): k = 3, padding 2, and a contiguous x, matching channels and a well-formed bias."""
    def tup(v):
        return (v,) * 3 if isinstance(v, int) else tuple(v)
    if not (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 5):
        return None
    k = weight.shape[2]
    if weight.shape[3] != k or weight.shape[4] != k or groups != 1 or tup(stride) != (1, 1, 1):
        return None
    if tup(dilation) == (1, 1, 1):
        if isinstance(padding, str) or tup(padding) != (k // 2,) * 3:
            return None
        return 1 if (k in (1, 3) or (k == 5 and weight.shape[1] == 1 and weight.shape[0] <= 64)) else None
    if _setting.dilated != CONV_DILATED_M3D or tup(dilation) != (2, 2, 2) or isinstance(padding, str) or tup(padding) != (2, 2, 2):
        return None
    if not (k == 3 and weight.is_cuda and weight.dim() == 5 and x.is_contiguous() and weight.shape[1] == x.shape[1]):
        return None
    if bias is not None and not (torch.is_tensor(bias) and bias.is_cuda and bias.dtype == torch.float32
                                 and tuple(bias.shape) == (weight.shape[0],)):
        return None
    return 2


def conv3d(input, weight, bias=None, stride=1, padding=0, dilation=1, groups=1):
    routed = _routed_dilation(input, weight, bias, stride, padding, dilation, groups)
    if routed is not None:
        return _Conv3dFn.apply(input.contiguous(), weight, bias, routed)        # (.contiguous(): dilation 1 only, a dilation-2 input already is)
    # a direct call (train.MaskHead) before install_conv3d(): torch's own is still in its place
    orig = _orig_conv3d if _orig_conv3d is not None else torch.nn.functional.conv3d
    return orig(input, weight, bias, stride, padding, dilation, groups)


# ----------------------------------------------------------------------------- F.linear interception (box head: fast_rcnn_heads.py:84-85,114-117,42-45)
_orig_linear = None
_lin_cache = {}           # id(parameter) -> (weakref, _version, data_ptr, bias id / version, SplitLinear)


def _split_linear(weight, bias):
    """bf16x3 pack of an nn.Linear weight, cached like the conv packs: only for live nn.Parameters at the same version / address."""
    if not isinstance(weight, torch.nn.Parameter):
        return ops.SplitLinear(weight.detach(), None if bias is None else bias.detach())
    bkey = None if bias is None else (id(bias), bias._version, bias.data_ptr())
    ent = _lin_cache.get(id(weight))
    if ent is not None:
        ref, ver, ptr, bk, lin = ent
        if ref() is weight and ver == weight._version and ptr == weight.data_ptr() and bk == bkey:
            return lin
    lin = ops.SplitLinear(weight.detach(), None if bias is None else bias.detach())
    _lin_cache[id(weight)] = (weakref.ref(weight, lambda _r, k=id(weight): _lin_cache.pop(k, None)), weight._version, weight.data_ptr(), bkey, lin)
    return lin


_linear_backward = (conv_plan.LINEAR_BACKWARD_FP32, None)      # set_linear_backward: (mode, min_work or None = the planner's constant)
_wmax_cache = {}          # id(parameter) -> (weakref, _version, data_ptr, max|W| as a 1-element device tensor)


def set_linear_backward(mode, min_work=None):
    """The backward of the intercepted nn.Linear layers: "fp32" (the default; install() does not change it) keeps m3d_linear_dgrad /
    m3d_linear_wgrad; "f16x2" takes m3d_linear_dgrad_f16x2 / m3d_linear_wgrad_f16x2 (csrc/fc_backward_f16.hip: the f16 matrix cores at
    fp32 accuracy, operands cut while they are staged) for the layers conv_plan.linear_backward_kernel routes to them.  gy is swept once
    per backward and its bound shared by both GEMMs, max|W| is cached per parameter like the packs (invalidate_packs() drops it), x is
    swept by the wgrad call.  The forward keeps its kernel and its bits.  min_work: the routing threshold in M N K (None:
    conv_plan.LINEAR_BACKWARD_F16X2_MIN_WORK; 0 routes every supported layer - tests and A/B runs).  Read when the backward runs.
    Returns the previous mode."""
    global _linear_backward
    if mode not in (conv_plan.LINEAR_BACKWARD_FP32, conv_plan.LINEAR_BACKWARD_F16X2):
        raise ValueError("set_linear_backward(%r): 'fp32' or 'f16x2'" % (mode,))
    prev, _linear_backward = _linear_backward[0], (mode, _threshold("set_linear_backward", "min_work", min_work))
    return prev


def get_linear_backward():
    return _linear_backward[0]


def _weight_max(weight):
    """max|W| of an nn.Linear weight as a 1-element device tensor, cached like _split_linear's packs: only for live nn.Parameters at the
    same version / address"""
    if not isinstance(weight, torch.nn.Parameter):
        return ops.absmax(weight.detach())
    ent = _wmax_cache.get(id(weight))
    if ent is not None:
        ref, ver, ptr, wmax = ent
        if ref() is weight and ver == weight._version and ptr == weight.data_ptr():
            return wmax
    wmax = ops.absmax(weight.detach())
    _wmax_cache[id(weight)] = (weakref.ref(weight, lambda _r, k=id(weight): _wmax_cache.pop(k, None)), weight._version, weight.data_ptr(), wmax)
    return wmax


class _LinearFn(torch.autograd.Function):
    """x [M,K] . W[N,K]^T + b on libm3d's GEMMs: the bf16x3 split kernels (fp32 accuracy) where K % 32 == 0 and N >= 64 (fc1, fc2),
    else the fp32-input MFMA kernel (cls_score, bbox_pred).  Backward (training; off the inference path): libm3d's dgrad and wgrad
    GEMMs on the saved operands as they are (csrc/fc_backward.hip) - no transposed copy, the bias gradient out of the wgrad launch;
    under set_linear_backward("f16x2") the same two GEMMs of csrc/fc_backward_f16.hip where conv_plan.linear_backward_kernel says so."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        if ops.SplitLinear.supported(weight):
            return _split_linear(weight, bias)(x)
        return ops.linear(x, weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = gb = None
        want_gb = ctx.has_bias and ctx.needs_input_grad[2]
        mode, min_work = _linear_backward
        if conv_plan.linear_backward_kernel(gy.shape[0], gy.shape[1], x.shape[1], mode, min_work) == conv_plan.LINEAR_BACKWARD_F16X2:
            gy_max = ops.absmax(gy)                                # one sweep, both GEMMs
            if ctx.needs_input_grad[0]:
                gx = ops.linear_dgrad_f16x2(gy, weight.detach(), gy_max, _weight_max(weight))
            if ctx.needs_input_grad[1] or want_gb:
                gw, gb = ops.linear_wgrad_f16x2(gy, x.detach(), gy_max, None, bias=want_gb)
                if not ctx.needs_input_grad[1]:
                    gw = None
            return gx, gw, gb
        if ctx.needs_input_grad[0]:
            gx = ops.linear_dgrad(gy, weight.detach())
        if ctx.needs_input_grad[1] or want_gb:
            gw, gb = ops.linear_wgrad(gy, x.detach(), bias=want_gb)
            if not ctx.needs_input_grad[1]:
                gw = None
        return gx, gw, gb


def _aligned16(t):
    return t.data_ptr() % 16 == 0 and t.is_contiguous()


def linear(input, weight, bias=None):
    # libm3d's GEMMs read 16-byte quads: K % 4 == 0 and 16-byte aligned, contiguous operands (a view into the middle of a
    # buffer goes to torch's own linear instead of raising M3D_EUNSUPPORTED)
    if (input.is_cuda and input.dtype == torch.float32 and weight.dtype == torch.float32 and input.dim() == 2 and weight.dim() == 2
            and input.shape[1] == weight.shape[1] and input.shape[1] % 4 == 0 and input.shape[0] > 0 and _aligned16(weight)):
        x = input.contiguous()
        if x.data_ptr() % 16 == 0:
            return _LinearFn.apply(x, weight, bias)
    return _orig_linear(input, weight, bias)


def invalidate_packs():
    """Drop every cached weight pack (conv and linear).  The caches are keyed on the parameter's `_version`, which in-place
    updates through `.data` (`p.data.mul_()`, `p.data.copy_()`, old-style optimisers) do NOT bump: call this after such an update,
    or update through the parameter itself (`with torch.no_grad(): p.mul_()`, `load_state_dict`), which does."""
    _pack_cache.clear()
    _lin_cache.clear()
    _wmax_cache.clear()
    _upconv_wmax_cache.clear()


def install_linear():
    global _orig_linear
    if _orig_linear is None:
        _orig_linear = torch.nn.functional.linear
        torch.nn.functional.linear = linear


def uninstall_linear():
    global _orig_linear
    if _orig_linear is not None:
        torch.nn.functional.linear = _orig_linear
        _orig_linear = None


def install_conv3d():
    global _orig_conv3d
    if _orig_conv3d is None:
        _orig_conv3d = torch.nn.functional.conv3d
        torch.nn.functional.conv3d = conv3d


def uninstall_conv3d():
    global _orig_conv3d
    if _orig_conv3d is not None:
        torch.nn.functional.conv3d = _orig_conv3d
        _orig_conv3d = None


# ----------------------------------------------------------------------------- F.batch_norm interception (opt-in; install() leaves it alone)
_orig_batch_norm = None


def batch_norm(input, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5):
    """fp32 CUDA contiguous [N,C,D,H,W] inputs go to m3d.batch_norm_relu(relu=False, pool=False) (csrc/bn_train.hip); everything else -
    and what that kernel refuses (C > 4096, 2^31 values per channel or more, a single value per channel) - to torch's own."""
    if (torch.is_tensor(input) and input.is_cuda and input.dtype == torch.float32 and input.dim() == 5 and input.is_contiguous()
            and input.shape[1] <= 4096 and 2 <= input.numel() // max(input.shape[1], 1) < 2 ** 31
            and (training or (running_mean is not None and running_var is not None))
            and all(t is None or (t.is_cuda and t.dtype == torch.float32 and tuple(t.shape) == (input.shape[1],) and t.is_contiguous())
                    for t in (running_mean, running_var, weight, bias))):
        from .train import batch_norm_relu
        return batch_norm_relu(input, weight, bias, running_mean, running_var, training, momentum, eps, relu=False, pool=False)
    return _orig_batch_norm(input, running_mean, running_var, weight, bias, training, momentum, eps)


def install_batch_norm():
    global _orig_batch_norm
    if _orig_batch_norm is None:
        _orig_batch_norm = torch.nn.functional.batch_norm
        torch.nn.functional.batch_norm = batch_norm


def uninstall_batch_norm():
    global _orig_batch_norm
    if _orig_batch_norm is not None:
        torch.nn.functional.batch_norm = _orig_batch_norm
        _orig_batch_norm = None


# ----------------------------------------------------------------------------- mask-head up-conv (opt-in; install() leaves it alone)
UPCONV_TORCH, UPCONV_M3D = "torch", "m3d"
_upconv = UPCONV_TORCH
_orig_conv_transpose3d = None


def set_upconv(mode):
    """The ConvTranspose3d(2, 2) + ReLU of the mask heads (train.MaskHead.forward, mask_head.MaskHeadM3D.up): "torch" (the default;
    install() does not change it) keeps torch's ConvTranspose3d and a separate ReLU in training, and the 1x1x1 conv to 8 Cout channels
    plus voxel shuffle at inference; "m3d" takes csrc/upconv3d.hip in both (m3d.upconv3d_2x: bias and ReLU in the epilogue, no
    intermediate, the library's dgrad / wgrad behind it; DESIGN, "Mask-head up-conv").  Returns the previous mode."""
    global _upconv
    if mode not in (UPCONV_TORCH, UPCONV_M3D):
        raise ValueError("set_upconv(%r): 'torch' or 'm3d'" % (mode,))
    prev, _upconv = _upconv, mode
    return prev


def get_upconv():
    return _upconv


_upconv_f16 = False


def set_upconv_f16(on):
    """The FORWARD of m3d.upconv3d_2x (train.MaskHead under set_upconv("m3d")) on the f16 matrix cores (ops.UpConvF16, csrc/upconv3d_f16.hip:
    the f16x2 cut at fp32 accuracy, one bound sweep of x per call, the pack served through the pack cache) where the kernel takes the
    shape (Cin % 16 == 0); the backward follows set_upconv_backward (fp32 by default), and takes the ReLU mask from the saved output whichever
    kernel wrote it.  Off by default, install() does not touch it, and it has no effect without set_upconv("m3d").  Returns the
    previous setting."""
    global _upconv_f16
    prev, _upconv_f16 = _upconv_f16, bool(on)
    return prev


def get_upconv_f16():
    return _upconv_f16


_upconv_backward = (conv_plan.UPCONV_BACKWARD_FP32, None)     # set_upconv_backward: (mode, min_work or None = the planner's constants)
_upconv_wmax_cache = {}   # id(parameter) -> (weakref, _version, data_ptr, max|W| as [ZwConv3d.SLOTS] device floats)


def set_upconv_backward(mode, min_work=None):
    """The BACKWARD of m3d.upconv3d_2x (train.MaskHead under set_upconv("m3d")): "fp32" (the default; install() does not touch it) keeps
    m3d_upconv3d_2x_dgrad / _wgrad; "f16x2" takes m3d_upconv3d_2x_dgrad_f16x2 / _wgrad_f16x2 (csrc/upconv3d_bwd_f16.hip: the f16 matrix
    cores at fp32 accuracy, gy, the ReLU mask, x and the weight read as they are and cut while they are staged) for each direction
    conv_plan.upconv_backward_kernel routes to them.  gy is swept once per backward and its bound shared by both passes, max|W| is
    cached per parameter like the packs (invalidate_packs() drops it, so Solver.step() does), x's bound is the one the f16x2 forward
    held where it ran, else the wgrad call sweeps x.  The forward keeps its kernel and its bits.  min_work: the routing threshold of
    both directions in multiply-adds R D H W Cin 8 Cout (None: conv_plan.UPCONV_BWD_F16_MIN_DGRAD / _WGRAD; 0 routes every supported
    shape - tests and A/B runs).  No effect without set_upconv("m3d").  Read when the backward runs.  Returns the previous mode."""
    global _upconv_backward
    if mode not in (conv_plan.UPCONV_BACKWARD_FP32, conv_plan.UPCONV_BACKWARD_F16X2):
        raise ValueError("set_upconv_backward(%r): 'fp32' or 'f16x2'" % (mode,))
    prev, _upconv_backward = _upconv_backward[0], (mode, _threshold("set_upconv_backward", "min_work", min_work))
    return prev


def get_upconv_backward():
    return _upconv_backward[0]


def _upconv_weight_max(weight):
    """max|W| of the up-conv's weight as [ZwConv3d.SLOTS] device floats, cached like _weight_max: only for live nn.Parameters at the
    same version / address"""
    if not isinstance(weight, torch.nn.Parameter):
        return ops.ZwConv3d.bound_of(weight.detach())
    ent = _upconv_wmax_cache.get(id(weight))
    if ent is not None:
        ref, ver, ptr, wmax = ent
        if ref() is weight and ver == weight._version and ptr == weight.data_ptr():
            return wmax
    wmax = ops.ZwConv3d.bound_of(weight.detach())
    _upconv_wmax_cache[id(weight)] = (weakref.ref(weight, lambda _r, k=id(weight): _upconv_wmax_cache.pop(k, None)), weight._version,
                                      weight.data_ptr(), wmax)
    return wmax


def _upconv_qualifies(x, weight, bias, stride, padding, output_padding, groups, dilation):
    def tup(v):
        return (v,) * 3 if isinstance(v, int) else tuple(v)
    if not (torch.is_tensor(x) and torch.is_tensor(weight) and x.is_cuda and weight.is_cuda and x.dtype == torch.float32
            and weight.dtype == torch.float32 and x.dim() == 5 and x.is_contiguous() and weight.dim() == 5):
        return False
    if tuple(weight.shape[2:]) != (2, 2, 2) or weight.shape[0] != x.shape[1] or groups != 1:
        return False
    if bias is not None and not (torch.is_tensor(bias) and bias.is_cuda and bias.dtype == torch.float32
                                 and tuple(bias.shape) == (weight.shape[1],)):
        return False
    return (tup(stride) == (2, 2, 2) and not isinstance(padding, str) and tup(padding) == (0, 0, 0) and tup(output_padding) == (0, 0, 0)
            and tup(dilation) == (1, 1, 1))


def conv_transpose3d(input, weight, bias=None, stride=1, padding=0, output_padding=0, groups=1, dilation=1):
    """Contiguous fp32 CUDA [R,Cin,D,H,W] inputs with a 2^3 kernel, stride 2, padding 0, output_padding 0, groups 1, dilation 1 go to
    m3d.upconv3d_2x (csrc/upconv3d.hip, forward and backward); everything else to torch's own with the original arguments."""
    if _upconv_qualifies(input, weight, bias, stride, padding, output_padding, groups, dilation):
        from .train import upconv3d_2x
        return upconv3d_2x(input, weight, bias, relu=False)
    orig = _orig_conv_transpose3d if _orig_conv_transpose3d is not None else torch.nn.functional.conv_transpose3d
    return orig(input, weight, bias, stride, padding, output_padding, groups, dilation)


def install_conv_transpose3d():
    global _orig_conv_transpose3d
    if _orig_conv_transpose3d is None:
        _orig_conv_transpose3d = torch.nn.functional.conv_transpose3d
        torch.nn.functional.conv_transpose3d = conv_transpose3d


def uninstall_conv_transpose3d():
    global _orig_conv_transpose3d
    if _orig_conv_transpose3d is not None:
        torch.nn.functional.conv_transpose3d = _orig_conv_transpose3d
        _orig_conv_transpose3d = None


# ----------------------------------------------------------------------------- registration
def _mod(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__m3d__ = True
    sys.modules[name] = m
    parent, _, child = name.rpartition(".")
    if parent and parent in sys.modules:
        setattr(sys.modules[parent], child, m)
    return m


def _pkg(name):
    """The real package when the reference's lib/ is importable, else an empty stand-in package."""
    if name not in sys.modules:
        try:
            importlib.import_module(name)
        except Exception:
            m = _mod(name)
            m.__path__ = []
    return sys.modules[name]


def install(conv3d=True, linear=True):
    """Register the drop-in modules.  Packages that already exist (the reference's `modeling`, `utils`) are kept;
    only the native-op leaf modules are replaced."""
    for pk in ("modeling", "modeling.roi_xfrom", "modeling.roi_xfrom.roi_align_3d",
               "modeling.roi_xfrom.roi_align_3d.functions", "modeling.roi_xfrom.roi_align_3d.modules",
               "utils", "model", "model.roi_pooling", "model.roi_pooling.functions", "model.roi_crop",
               "model.roi_crop.functions"):
        _pkg(pk)
    _mod("modeling.roi_xfrom.roi_align_3d.functions.roi_align_3d", RoIAlignFunction_3d=RoIAlignFunction_3d)
    _mod("modeling.roi_xfrom.roi_align_3d.modules.roi_align_3d", RoIAlign_3d=RoIAlign_3d, RoIAlignAvg_3d=RoIAlignAvg_3d,
         RoIAlignMax_3d=RoIAlignMax_3d, RoIAlignFunction_3d=RoIAlignFunction_3d)
    _mod("utils.cython_nms_3d", nms_3d=nms_3d, nms_3d_volume=nms_3d_volume, soft_nms_3d=soft_nms_3d)
    _mod("utils.cython_bbox_3d", bbox_overlaps_3d=bbox_overlaps_3d)
    _mod("model.roi_pooling.functions.roi_pool", RoIPoolFunction=_Legacy2D)
    _mod("model.roi_crop.functions.roi_crop", RoICropFunction=_Legacy2D)
    try:                                   # tools/otsu.py also holds otsu_py / otsu_py_2d (binarization_nuclei.py:12)
        importlib.import_module("otsu").otsu_py_2d_fast = otsu_py_2d_fast
    except Exception:
        _mod("otsu", otsu_py_2d_fast=otsu_py_2d_fast)
    if conv3d:
        install_conv3d()
    if linear:
        install_linear()
