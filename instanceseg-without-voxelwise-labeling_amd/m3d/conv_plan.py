"""Which kernel runs a backbone / RPN convolution, decided in one place, and the per-layer object that runs the decision.

`plan_conv` is the only place the order of the kernel families lives (DESIGN.md "Conv dispatch"): the detection path
(DetectorM3D.body_layer / rpn), bench.py's roofline bookkeeping (DetectorM3D.conv_work) and the PRM forward
(PRMEngine.forward_response) all ask it, each with its own needs, and run what it says by calling the layer's `LayerConv`.

`plan_train_conv` is the same for the training path (m3d.compat.conv3d and its backward): everything the switches of m3d.compat say
travels as one `TrainSetting` (FORWARD_FIELDS / BACKWARD_FIELDS: when each field is read), the rules `train_conv_kernel` and
`wgrad_kernel` are its rows, and `compat._Conv3dFn` runs the plan from two tables keyed by its kinds (DESIGN.md "Training conv
dispatch")."""
import collections

import torch

from . import ops

# The Winograd, stem and f16x2 kernels address one batch item with 32-bit buffer offsets: an item of this many bytes or more runs on
# the direct kernel.
ITEM_LIMIT = 0x7FFFFFFF
# The f16x2 kernel runs one workgroup per (64 channels, 32 x 4 x 2 voxels): maps that give it less than ~0.8 of a round of the chip's
# 256 CUs stay with the fp32 Winograd kernels (split-K over workgroups).
ZW_MIN_UNITS = 200

DIRECT, STEM, ZW = "direct", "winograd F(2,5)x stem", "f16x2 F(2,3)z"         # kinds: keys of DetectorM3D.ISSUED_FRACTION
ZN = "f16x2 narrow"                   # csrc/conv3d_zn.hip: maps at most 8 wide (the per-RoI convs), opt-in (narrow_f16)
# The narrow f16x2 kernel runs one workgroup per (64 channels, 8 x 8 x 4 voxels); a 7^3 RoI grid is 2 units per RoI and 64 channels.
# Every row of profiles/conv_narrow_f16.txt is faster than the direct fp32 kernel by more than the spreads, sweep / gy_reduce and the
# per-step pack inside the window: 1.9 x .. 3.2 x from 512 units up, and the two smallest launches measured, 128 units (the mask head's
# 256 -> 256 at R = 16, forward and dgrad), still 1.17 x and 1.13 x.  Nothing smaller was measured: it stays on fp32.
ZN_MIN_UNITS = 128

# kind: the kernel family; fused: the layer's max-pool runs in the conv launch (else ops.maxpool3d_2x follows); sweep: the kernel scales
# its input by the input's operand bound (DetectorM3D._bound: left on the tensor by the launch that produced it, else one sweep)
Plan = collections.namedtuple("Plan", "kind fused sweep")

WGRAD_FP32, WGRAD_F16X2 = "fp32", "f16x2"            # wgrad kernels: m3d_conv3d_wgrad / m3d_conv3d_wgrad_f16x2 (+ its two bound sweeps)
# The f16x2 weight gradient pays two sweeps of its operands, a workspace round trip of 27 cin cout floats per slot and a second launch:
# fixed costs that a layer's work, batch x voxels x cin x cout products per tap, has to carry.  A layer is routed to it from the work of
# the smallest layer measured to win by more than the spread (profiles/conv_wgrad_f16.txt: conv4a of the stride-8 body on one 128^3
# volume, 16^3 x 128 x 256 = 2^27, 2.2 x); every measured layer above it wins too (1.3 x .. 2.2 x).  Below it nothing routes.
WGRAD_F16X2_MIN_WORK = 1 << 27


# The dilation-1 fp32 kernel on the 2 x 8 x 8 voxel tile (m3d_conv3d_wgrad_narrow): maps at most 8 wide, i.e. the per-RoI convs on 7^3
# grids of the conv box head and of the mask head at MRCNN.DILATION = 1.  Opt-in (compat.set_conv_wgrad_narrow).
WGRAD_NARROW = "fp32 narrow"
# The f16x2 cut on that 2 x 8 x 8 tile (m3d_conv3d_wgrad_narrow_f16x2): opt-in (compat.set_conv_wgrad_narrow_f16).
WGRAD_NARROW_F16X2 = "f16x2 narrow"
# Its fixed costs are the wide kernel's (two sweeps where the step holds no bound, a workspace round trip per slot, a second launch).  A
# layer is routed to it from the work, batch x voxels x cin x cout products per tap, of the smallest shape measured to beat the faster of
# m3d_conv3d_wgrad_narrow and m3d_conv3d_wgrad_f16x2 by more than the sum of the spreads, sweeps inside the window
# (profiles/conv_wgrad_narrow_f16.txt: 256 -> 256 on 7^3 at R = 4, 4 x 343 x 256 x 256, 1.58 x); all eleven larger measured shapes win
# too (1.92 x .. 2.32 x).  Nothing smaller was measured: below it nothing routes.
WGRAD_NARROW_F16X2_MIN_WORK = 4 * 343 * 256 * 256


def wgrad_kernel(batch, cin, cout, D, H, W, mode, k=3, narrow=False, narrow_f16=None):
    """Which kernel computes the weight gradient of a stride-1 'same' conv layer with x [batch, cin, D, H, W]: WGRAD_F16X2, WGRAD_NARROW,
    WGRAD_NARROW_F16X2 or WGRAD_FP32.  The one place that says so (a row of plan_train_conv).  mode: the caller's setting (compat.set_conv_wgrad):
    "fp32" keeps every layer on m3d_conv3d_wgrad; "f16x2" moves the layers the f16x2 kernel takes (k = 3, cin and cout multiples of 32:
    m3d_conv3d_wgrad_f16x2_supported) and was measured to win on by more than the spread of the measurement: layers of at least
    WGRAD_F16X2_MIN_WORK products per tap.  narrow: the caller's switch (compat.set_conv_wgrad_narrow): a k = 3 layer that would end on
    WGRAD_FP32 and that m3d_conv3d_wgrad_narrow takes (W <= 8) is WGRAD_NARROW instead; a layer the mode routes to f16x2 stays there.
    narrow_f16: None (off: the result is what it was without the argument, and no further library query is made), else a routing
    threshold in products per tap (compat.set_conv_wgrad_narrow_f16): a k = 3 layer that m3d_conv3d_wgrad_narrow_f16x2_supported takes
    (W <= 8, cin and cout multiples of 32) and whose work reaches it is WGRAD_NARROW_F16X2 whatever mode and narrow say - at W <= 8
    the wide f16x2 tile is a third full; every other layer follows the rule above.
    A function of the shape only."""
    if mode not in (WGRAD_FP32, WGRAD_F16X2):
        raise ValueError("wgrad mode %r: 'fp32' or 'f16x2'" % (mode,))
    if int(k) != 3:
        return WGRAD_FP32
    if (narrow_f16 is not None and ops.conv3d_wgrad_narrow_f16x2_supported(batch, cin, cout, D, H, W)
            and int(batch) * int(D) * int(H) * int(W) * int(cin) * int(cout) >= int(narrow_f16)):
        return WGRAD_NARROW_F16X2
    if (mode == WGRAD_F16X2 and ops.conv3d_wgrad_f16x2_supported(batch, cin, cout, D, H, W)
            and int(batch) * int(D) * int(H) * int(W) * int(cin) * int(cout) >= WGRAD_F16X2_MIN_WORK):
        return WGRAD_F16X2
    if narrow and ops.conv3d_wgrad_narrow_supported(batch, cin, cout, D, H, W, 3):
        return WGRAD_NARROW
    return WGRAD_FP32


LINEAR_BACKWARD_FP32, LINEAR_BACKWARD_F16X2 = "fp32", "f16x2"    # nn.Linear backward: csrc/fc_backward.hip / csrc/fc_backward_f16.hip
# The f16x2 backward pays a sweep of gy and of x per step and one of the weight per parameter version; a layer is routed to it from the
# work M N K of the smallest row of profiles/linear_backward_f16.txt whose backward (dgrad + wgrad, the gy and x sweeps inside the
# window, the weight's bound cached) beat the fp32 kernels by more than the sum of the two spreads: fc1 at the nuclei K with 64 rows,
# 64 x 1024 x 87 808 (0.250 against 0.456 ms, 1.83 x); the four larger rows win too (1.89 x .. 2.17 x), and the one smaller row, fc2
# (128 x 1024 x 1024), LOSES (0.053 against 0.037 ms: three more launches than it has work for).  Nothing smaller routes by default.
LINEAR_BACKWARD_F16X2_MIN_WORK = 64 * 1024 * 87808


def linear_backward_kernel(M, N, K, mode, min_work=None):
    """Which kernels compute the backward of an nn.Linear with gy [M, N], weight [N, K]: LINEAR_BACKWARD_FP32 (m3d_linear_dgrad /
    m3d_linear_wgrad) or LINEAR_BACKWARD_F16X2 (m3d_linear_dgrad_f16x2 / m3d_linear_wgrad_f16x2).  The one place that says so.  mode: the
    caller's setting (compat.set_linear_backward): "fp32" keeps every layer where it is; "f16x2" moves the layers that
    m3d_linear_backward_f16x2_supported takes (N >= 64, N and K multiples of 4: fc1 and fc2, never cls_score / bbox_pred) and whose work
    M N K reaches min_work (None: LINEAR_BACKWARD_F16X2_MIN_WORK; 0: every supported layer).  A function of the shape only."""
    if mode not in (LINEAR_BACKWARD_FP32, LINEAR_BACKWARD_F16X2):
        raise ValueError("linear backward mode %r: 'fp32' or 'f16x2'" % (mode,))
    if mode == LINEAR_BACKWARD_FP32:
        return LINEAR_BACKWARD_FP32
    floor = LINEAR_BACKWARD_F16X2_MIN_WORK if min_work is None else int(min_work)
    if int(M) * int(N) * int(K) >= floor and ops.linear_backward_f16x2_supported(M, N, K):
        return LINEAR_BACKWARD_F16X2
    return LINEAR_BACKWARD_FP32


UPCONV_BACKWARD_FP32, UPCONV_BACKWARD_F16X2 = "fp32", "f16x2"    # up-conv backward: csrc/upconv3d.hip / csrc/upconv3d_bwd_f16.hip
# Routing thresholds of the up-conv's f16x2 backward per direction, in multiply-adds of the GEMM, R D H W x Cin x 8 Cout: the work of
# the smallest row of profiles/upconv_backward_f16.txt (256 -> 256 channels, 7^3 -> 14^3, ReLU mask, the gy sweep inside the window,
# max|W| cached) at which the f16x2 call beat m3d_upconv3d_2x_dgrad / _wgrad by more than the sum of the two spreads.  None: the
# direction was never measured to win and does not route by default.  Nothing smaller than a measured win routes.
#   dgrad: wins at R = 64 (0.239 against 0.327 ms, x1.37) and R = 300 (0.908 against 1.274 ms, x1.40); LOSES at R = 16 (0.133 against
#          0.085 ms: 86 workgroups on 256 CUs, and the sweep is a launch of its own) and R = 4 (0.130 against 0.039 ms).
#   wgrad: LOSES at every measured count (R = 4, 16, 64, 300: x0.76, x0.84, x0.73, x0.58 - the 4- and 8-byte gathers of x and gy along
#          the reduction bound it at 0.8 - 0.9 TB/s of gy + y): it never routes by default.
UPCONV_BWD_F16_MIN_DGRAD = 64 * 343 * 256 * 8 * 256
UPCONV_BWD_F16_MIN_WGRAD = None
UPCONV_BWD_F16_MIN = {"dgrad": UPCONV_BWD_F16_MIN_DGRAD, "wgrad": UPCONV_BWD_F16_MIN_WGRAD}


def upconv_backward_kernel(direction, R, Cin, Cout, D, H, W, setting):
    """Which kernel computes the "dgrad" or the "wgrad" (+ bias gradient) of the mask head's ConvTranspose3d(2, 2) with x [R,Cin,D,H,W]
    and weight [Cin,Cout,2,2,2]: UPCONV_BACKWARD_FP32 (m3d_upconv3d_2x_dgrad / _wgrad) or UPCONV_BACKWARD_F16X2
    (m3d_upconv3d_2x_dgrad_f16x2 / _wgrad_f16x2).  The one place that says so.  setting: (mode, min_work) as compat.set_upconv_backward
    keeps it - mode "fp32" keeps both directions where they are; "f16x2" moves a direction whose shape
    m3d_upconv3d_2x_backward_f16x2_supported takes (Cin and Cout multiples of 32) and whose work R D H W Cin 8 Cout reaches min_work
    (None: the direction's UPCONV_BWD_F16_MIN_* constant, and no routing where that is None; 0: every supported shape).  A function of
    the shape only."""
    if direction not in UPCONV_BWD_F16_MIN:
        raise ValueError("direction %r: 'dgrad' or 'wgrad'" % (direction,))
    mode, min_work = setting
    if mode not in (UPCONV_BACKWARD_FP32, UPCONV_BACKWARD_F16X2):
        raise ValueError("up-conv backward mode %r: 'fp32' or 'f16x2'" % (mode,))
    if mode == UPCONV_BACKWARD_FP32:
        return UPCONV_BACKWARD_FP32
    floor = UPCONV_BWD_F16_MIN[direction] if min_work is None else int(min_work)
    if floor is None:
        return UPCONV_BACKWARD_FP32
    R, Cin, Cout, D, H, W = (int(v) for v in (R, Cin, Cout, D, H, W))
    if R * D * H * W * Cin * 8 * Cout >= floor and ops.upconv3d_2x_backward_f16x2_supported((R, Cin, D, H, W), Cout):
        return UPCONV_BACKWARD_F16X2
    return UPCONV_BACKWARD_FP32


TRAIN_FP32, TRAIN_F16X2 = "fp32", "f16x2"            # forward / dgrad kernels of a training conv: the direct fp32 MFMA kernel / conv3d_zw.hip
TRAIN_F16X2_NARROW = "f16x2 narrow"                  # conv3d_zn.hip (ops.ZnConv3d): maps at most 8 wide, opt-in (compat.set_conv_train_narrow)
# Output channels of the launched conv (forward: cout; dgrad: the forward cin) from which a direction routes to the f16x2 kernel.  Its
# units are 64 channels wide: with 32 output channels half of every unit's matrix work is spent on channels that do not exist.  The PRM
# engine keeps such a dgrad off the kernel (PRMEngine._dgrad_zw: >= 64, measured against the fp32 Winograd strips); against the DIRECT
# fp32 kernel of the training path the half-idle 64 -> 32 launch (conv2a's dgrad) still won 3.5 x .. 4.6 x on every map that fills the
# chip (profiles/conv_train_f16.txt), so 32 is admitted in both directions.  Nothing narrower was measured: it stays on fp32.
# The unit threshold is ZW_MIN_UNITS as for the detection path: every measured launch of 256 units or more won (2.2 x .. 5.6 x with the
# per-step pack inside the window), the two of 128 units won too (2.1 x, 2.3 x), those of 64 were mixed (0.89 x .. 2.9 x), none of 16 or fewer was faster than 1.03 x.
TRAIN_F16X2_MIN_COUT = {"forward": 32, "dgrad": 32}


def _narrow_takes(batch, ci, co, D, H, W, min_units):
    """the narrow f16x2 kernel takes the launched conv [batch, ci, D, H, W] -> co and the launch reaches min_units units"""
    L = ops.lib()
    if batch < 1 or ci < 1 or co < 1 or not L.m3d_conv3d_zn_supported(ci, co, D, H, W):
        return False
    return L.m3d_conv3d_zn_launch_units(batch, ci, co, D, H, W) >= int(min_units)


def train_conv_kernel(direction, batch, cin, cout, D, H, W, mode, min_units=ZW_MIN_UNITS, k=3, narrow=False, narrow_min_units=ZN_MIN_UNITS):
    """Which kernel runs the forward ("forward") or the backward-data ("dgrad") conv of a stride-1 'same' training layer with weight
    [cout, cin, k, k, k] on a map [batch, ., D, H, W]: TRAIN_F16X2 (m3d_conv3d_zw_forward; dgrad on an m3d_conv3d_zw_pack_dgrad pack) or
    TRAIN_FP32 (the direct fp32 MFMA kernel, ops.PackedConv3d).  The one place that says so (a row of plan_train_conv, as wgrad_kernel is).
    mode: the caller's setting (compat.set_conv_train).  TRAIN_FP32 for mode "fp32", k != 3, channel counts or a map the zw kernel has no
    configuration for (m3d_conv3d_zw_supported on the launched conv: a dgrad swaps the channel roles), a batch item of ITEM_LIMIT bytes
    or more, fewer launched output channels than TRAIN_F16X2_MIN_COUT[direction], fewer than min_units launch units.
    narrow: the caller's switch (compat.set_conv_train_narrow), independent of mode: a k = 3 layer the zw kernel does not take
    (m3d_conv3d_zw_supported refuses maps narrower than 12), that m3d_conv3d_zn_supported takes for the launched conv (W <= 8, launched
    input channels a multiple of 16) and whose launch has at least narrow_min_units units is TRAIN_F16X2_NARROW (ops.ZnConv3d; dgrad on its
    dgrad_of pack).  With narrow left False the result is what it was without the argument.  A function of the shape only."""
    if direction not in TRAIN_F16X2_MIN_COUT:
        raise ValueError("direction %r: 'forward' or 'dgrad'" % (direction,))
    if mode not in (TRAIN_FP32, TRAIN_F16X2):
        raise ValueError("conv train mode %r: 'fp32' or 'f16x2'" % (mode,))
    if int(k) != 3:
        return TRAIN_FP32
    batch, D, H, W = int(batch), int(D), int(H), int(W)
    ci, co = (int(cin), int(cout)) if direction == "forward" else (int(cout), int(cin))     # of the conv that is launched
    L = ops.lib()
    zw_takes = batch >= 1 and ci >= 1 and co >= 1 and bool(L.m3d_conv3d_zw_supported(ci, co, D, H, W, 0))
    if narrow and not zw_takes and _narrow_takes(batch, ci, co, D, H, W, narrow_min_units):
        return TRAIN_F16X2_NARROW
    if mode == TRAIN_FP32 or not zw_takes:
        return TRAIN_FP32
    # (m3d_conv3d_zw_forward itself refuses an item from 0x7FFFFF00 bytes: the 255 bytes below ITEM_LIMIT stay on fp32 too)
    if ci * D * H * W * 4 >= ITEM_LIMIT - 0xFF or co < TRAIN_F16X2_MIN_COUT[direction]:
        return TRAIN_FP32
    if L.m3d_conv3d_zw_launch_units(batch, ci, co, D, H, W) < int(min_units):
        return TRAIN_FP32
    return TRAIN_F16X2


# ----------------------------------------------------------------------------- the training plan (m3d.compat._Conv3dFn runs it)
DILATED_TORCH, DILATED_M3D = "torch", "m3d"          # who runs the k = 3, dilation 2, padding 2 convs (compat.set_conv_dilated)
TRAIN_DILATED = "dilated"                            # forward / dgrad kind: m3d_conv3d_forward_dilated (fp32, on the W_PLAIN / W_DGRAD pack)
DGRAD_STEM = "stem"                                  # dgrad kind: the VALU kernel of the 5^3 / Cin = 1 stem (m3d_conv3d_stem5_dgrad)
WGRAD_DILATED = "dilated"                            # wgrad kind: m3d_conv3d_wgrad_dilated
GB_REDUCE, GB_BIAS_GRAD = "gy_reduce", "bias_grad"   # where the bias gradient comes from
# forward / dgrad kind: the dilation-2 instantiation of the narrow f16x2 kernel (m3d_conv3d_zn_dilated_forward; dgrad on the
# m3d_conv3d_zn_pack_dgrad pack): maps at most 8 wide under DILATED_M3D, opt-in (compat.set_conv_dilated_f16)
TRAIN_DILATED_F16X2 = "f16x2 dilated"
# Its routing threshold in launch units (64 channels x 8 x 8 x 4 voxels; a 7^3 RoI grid is 2 units per RoI and 64 channels): the unit
# count of the smallest launch of profiles/conv_narrow_f16_dilated.txt that beat m3d_conv3d_forward_dilated by more than the sum of the
# spreads, sweep / gy_reduce and the per-step pack inside the window.  Nothing below a measured win routes.
ZN_DILATED_MIN_UNITS = 128
# The mask head's tail (up-conv + ReLU + classifier + sigmoid) as ONE f16x2 launch (ops.UpConvF16.tail, csrc/upconv3d_f16.hip), opt-in
# (MaskHeadM3D(tail_f16=) / M3D_MASK_TAIL_F16).  Its routing threshold in RoIs: the smallest RoI count of profiles/mask_tail_f16.txt
# (256 -> 256 channels, 7^3 -> 14^3, K = 2) at which the fused call, its own bound sweep inside the window, beat the fp32 up-conv +
# classify conv + torch.sigmoid by more than the sum of the spreads (16 is the smallest count measured: x1.20 with the sweep, x1.47
# without).  Smaller launches do not route.
MASK_TAIL_F16_MIN_ROIS = 16
# wgrad kind: the dilation-2 instantiation of the narrow f16x2 wgrad kernel (m3d_conv3d_wgrad_narrow_dilated_f16x2): maps at most 8 wide,
# cin and cout multiples of 32, under DILATED_M3D, opt-in (compat.set_conv_wgrad_dilated_f16)
WGRAD_DILATED_F16X2 = "f16x2 dilated"
# Its routing threshold in products per tap, batch x voxels x cin x cout, as WGRAD_NARROW_F16X2_MIN_WORK is: the work of the smallest
# shape measured to beat m3d_conv3d_wgrad_dilated by more than the sum of the spreads, both operand sweeps inside the window
# (profiles/conv_wgrad_dilated_f16.txt: 256 -> 256 on 7^3 at R = 4, 4 x 343 x 256 x 256, 0.259 -> 0.101 ms, 2.56 x); all six larger
# measured shapes win too (2.66 x .. 3.12 x).  Nothing smaller was measured: below it nothing routes.
WGRAD_DILATED_F16X2_MIN_WORK = 4 * 343 * 256 * 256


class TrainSetting(collections.namedtuple(
        "TrainSetting", "train min_units narrow wgrad wgrad_narrow dilated wgrad_narrow_f16 dilated_f16 wgrad_dilated_f16",
        defaults=(TRAIN_FP32, None, None, WGRAD_FP32, False, DILATED_TORCH, None, None, None))):
    """Everything the switches of m3d.compat say about a training conv, immutable; the defaults are install()'s.
    | field             | value                                                                        | setter                     | read at  |
    | train             | TRAIN_FP32 / TRAIN_F16X2                                                     | set_conv_train             | forward  |
    | min_units         | its routing threshold in launch units; None: ZW_MIN_UNITS                    | set_conv_train             | forward  |
    | narrow            | None: the narrow f16x2 kernel is off; else its threshold in launch units     | set_conv_train_narrow      | forward  |
    | wgrad             | WGRAD_FP32 / WGRAD_F16X2                                                     | set_conv_wgrad             | backward |
    | wgrad_narrow      | bool                                                                         | set_conv_wgrad_narrow      | backward |
    | dilated           | DILATED_TORCH / DILATED_M3D                                                  | set_conv_dilated           | forward  |
    | wgrad_narrow_f16  | None: the narrow f16x2 wgrad is off; else its threshold in products per tap  | set_conv_wgrad_narrow_f16  | backward |
    | dilated_f16       | None: the dilation-2 f16x2 kernel is off; else its threshold in launch units | set_conv_dilated_f16       | forward  |
    | wgrad_dilated_f16 | None: the dilation-2 f16x2 wgrad is off; else its threshold in products/tap  | set_conv_wgrad_dilated_f16 | backward |
    "forward" (FORWARD_FIELDS): the value of the forward call - the conv Function keeps the forward's setting and its backward follows
    it, whatever the setters were told in between.  "backward" (BACKWARD_FIELDS): the value when the backward runs - the Function puts
    the current ones into the kept setting before it asks plan_train_backward."""
    __slots__ = ()


FORWARD_FIELDS = ("train", "min_units", "narrow", "dilated", "dilated_f16")
BACKWARD_FIELDS = ("wgrad", "wgrad_narrow", "wgrad_narrow_f16", "wgrad_dilated_f16")


# forward: TRAIN_FP32 / TRAIN_F16X2 / TRAIN_F16X2_NARROW / TRAIN_DILATED / TRAIN_DILATED_F16X2; sweep: the forward sweeps x for its operand bound and keeps it
# (for the f16x2 wgrad); dgrad: None (gx not needed) / DGRAD_STEM / TRAIN_FP32 / TRAIN_F16X2 / TRAIN_F16X2_NARROW / TRAIN_DILATED / TRAIN_DILATED_F16X2;
# wgrad: None (gw not needed) / WGRAD_FP32 / WGRAD_F16X2 / WGRAD_NARROW / WGRAD_NARROW_F16X2 / WGRAD_DILATED / WGRAD_DILATED_F16X2; gy_reduce: m3d_conv3d_gy_reduce runs first (one
# pass over gy: its operand bound, and the bias gradient where needed); gb: None / GB_REDUCE / GB_BIAS_GRAD
TrainConvPlan = collections.namedtuple("TrainConvPlan", "forward sweep dgrad wgrad gy_reduce gb")


def _train_rule(direction, setting, xshape, wshape):
    """train_conv_kernel's row for a dilation-1 layer with weight `wshape` on a map `xshape` under `setting`"""
    if setting.train == TRAIN_FP32 and setting.narrow is None:
        return TRAIN_FP32
    B, _, D, H, W = xshape
    kw = {} if setting.narrow is None else dict(narrow=True, narrow_min_units=setting.narrow)
    return train_conv_kernel(direction, B, wshape[1], wshape[0], D, H, W, setting.train,
                             min_units=ZW_MIN_UNITS if setting.min_units is None else setting.min_units, k=wshape[2], **kw)


def _dilated_takes(batch, ci, co, D, H, W, min_units):
    """the dilation-2 narrow f16x2 kernel takes the launched conv [batch, ci, D, H, W] -> co and the launch reaches min_units units"""
    L = ops.lib()
    if batch < 1 or ci < 1 or co < 1 or not L.m3d_conv3d_zn_dilated_supported(ci, co, D, H, W, 2):
        return False
    return L.m3d_conv3d_zn_dilated_launch_units(batch, ci, co, D, H, W, 2) >= int(min_units)


def _dilated_rule(direction, setting, xshape, wshape):
    """the forward / dgrad kind of a dilation-2 layer: TRAIN_DILATED_F16X2 where the switch is on (setting.dilated_f16: its threshold in
    launch units) under DILATED_M3D and the kernel takes the LAUNCHED conv (a dgrad swaps the channel roles, as train_conv_kernel does),
    else TRAIN_DILATED.  With dilated_f16 None no library query is made."""
    if setting.dilated_f16 is None or setting.dilated != DILATED_M3D or int(wshape[2]) != 3:
        return TRAIN_DILATED
    B, _, D, H, W = (int(v) for v in xshape)
    ci, co = (int(wshape[1]), int(wshape[0])) if direction == "forward" else (int(wshape[0]), int(wshape[1]))
    return TRAIN_DILATED_F16X2 if _dilated_takes(B, ci, co, D, H, W, setting.dilated_f16) else TRAIN_DILATED


def plan_train_forward(setting, xshape, wshape, dilation):
    """(forward, sweep) of plan_train_conv: what the forward of the call needs, and no library query beyond that"""
    if dilation == 2:
        forward = _dilated_rule("forward", setting, xshape, wshape)
        return forward, forward == TRAIN_DILATED_F16X2
    forward = _train_rule("forward", setting, xshape, wshape)
    return forward, forward != TRAIN_FP32


def _wgrad_dilated_rule(setting, xshape, wshape):
    """the wgrad kind of a dilation-2 layer: WGRAD_DILATED_F16X2 where the switch is on (setting.wgrad_dilated_f16: its threshold in
    products per tap) under DILATED_M3D, k = 3, m3d_conv3d_wgrad_narrow_dilated_f16x2_supported takes the shape at dilation 2 and the
    work reaches the threshold, else WGRAD_DILATED.  With wgrad_dilated_f16 None no library query is made."""
    if setting.wgrad_dilated_f16 is None or setting.dilated != DILATED_M3D or int(wshape[2]) != 3:
        return WGRAD_DILATED
    B, _, D, H, W = (int(v) for v in xshape)
    cout, cin = int(wshape[0]), int(wshape[1])
    if (ops.conv3d_wgrad_narrow_f16x2_supported(B, cin, cout, D, H, W, dilation=2)
            and B * D * H * W * cin * cout >= int(setting.wgrad_dilated_f16)):
        return WGRAD_DILATED_F16X2
    return WGRAD_DILATED


def plan_train_backward(setting, xshape, wshape, dilation, needs):
    """(dgrad, wgrad, gy_reduce, gb) of plan_train_conv: what the backward of the call needs.  A switch left at None changes nothing and
    asks the library nothing."""
    gx, gw, gb = (bool(v) for v in needs)
    if dilation == 2:                                  # train, wgrad and wgrad_narrow_f16 do not reach these layers
        dgrad = _dilated_rule("dgrad", setting, xshape, wshape) if gx else None
        gy_reduce = dgrad == TRAIN_DILATED_F16X2       # gy's bound, and then the bias gradient too: the rule of TRAIN_F16X2_NARROW
        # WGRAD_DILATED_F16X2 asks for nothing, as WGRAD_NARROW_F16X2 does not: it takes gy's bound where the pass ran and sweeps otherwise
        wgrad = _wgrad_dilated_rule(setting, xshape, wshape) if gw else None
        return dgrad, wgrad, gy_reduce, ((GB_REDUCE if gy_reduce else GB_BIAS_GRAD) if gb else None)
    B, _, D, H, W = xshape
    cout, cin, k = wshape[:3]
    dgrad = None if not gx else DGRAD_STEM if k == 5 else _train_rule("dgrad", setting, xshape, wshape)
    # base: the wgrad kernel without the narrow f16x2 switch (the only one asked while that switch is off)
    base = wgrad_kernel(B, cin, cout, D, H, W, setting.wgrad, k=k, narrow=setting.wgrad_narrow) if gw else None
    wgrad = base if base is None or setting.wgrad_narrow_f16 is None else \
        wgrad_kernel(B, cin, cout, D, H, W, setting.wgrad, k=k, narrow=setting.wgrad_narrow, narrow_f16=setting.wgrad_narrow_f16)
    # one pass over gy gives the bound both f16x2 kernels scale gy by, and the bias gradient.  In train mode f16x2 gb ALWAYS comes from
    # it, so that a change of route (another batch size, min_units) never changes gb; in mode fp32 only the narrow f16x2 dgrad asks for
    # it (the f16x2 wgrad then sweeps both operands itself).  WGRAD_NARROW_F16X2 asks for nothing: the pass runs where it would have run
    # for `base`, the wgrad kernel without wgrad_narrow_f16; the narrow kernel takes gy's bound where it ran and sweeps otherwise, so
    # gy_reduce and gb are the same with its switch on or off
    gy_reduce = (setting.train == TRAIN_F16X2 and (dgrad == TRAIN_F16X2 or base == WGRAD_F16X2 or gb)) or dgrad == TRAIN_F16X2_NARROW
    return dgrad, wgrad, gy_reduce, ((GB_REDUCE if gy_reduce else GB_BIAS_GRAD) if gb else None)


def plan_train_conv(setting, xshape, wshape, dilation, needs):
    """What a training conv that m3d.compat.conv3d routes to the library launches, forward and backward: a TrainConvPlan.  The only place
    that combines the rules (train_conv_kernel and wgrad_kernel are its rows); host queries of the library only, a function of its
    arguments only.  setting: a TrainSetting; xshape [B, cin, D, H, W]; wshape [cout, cin, k, k, k]; dilation: 1 (stride 1, padding
    k // 2, k in {1, 3} or the 5^3 / Cin = 1 stem) or 2 (k = 3, padding 2, only routed under DILATED_M3D); needs = (gx, gw, gb) of
    needs_input_grad, gb already False for a layer without bias.  setting.wgrad_narrow_f16 moves the wgrad field of dilation-1 layers
    only and setting.wgrad_dilated_f16 that of dilation-2 layers under DILATED_M3D only: gy_reduce and gb depend on neither.
    setting.dilated_f16 moves dilation-2 layers under DILATED_M3D only.  "dilated f16x2 takes": setting.dilated_f16 is a threshold,
    setting.dilated is DILATED_M3D, m3d_conv3d_zn_dilated_supported takes the LAUNCHED conv at dilation 2 (a dgrad swaps the channel
    roles) and m3d_conv3d_zn_dilated_launch_units reaches the threshold.

    | field     | value              | condition                                                                                      |
    | forward   | TRAIN_DILATED_F16X2| dilation 2 and dilated f16x2 takes the forward conv                                            |
    |           | TRAIN_DILATED      | dilation 2 otherwise                                                                           |
    |           | else               | train_conv_kernel("forward", ...) under setting.train / min_units / narrow                     |
    | sweep     | True               | forward is TRAIN_F16X2, TRAIN_F16X2_NARROW or TRAIN_DILATED_F16X2                              |
    | dgrad     | None               | gx not needed                                                                                  |
    |           | TRAIN_DILATED_F16X2| dilation 2 and dilated f16x2 takes the backward-data conv                                      |
    |           | TRAIN_DILATED      | dilation 2 otherwise                                                                           |
    |           | DGRAD_STEM         | k = 5                                                                                          |
    |           | else               | train_conv_kernel("dgrad", ...)                                                                |
    | wgrad     | None               | gw not needed                                                                                  |
    |           | WGRAD_DILATED_F16X2| dilation 2, setting.wgrad_dilated_f16 is a threshold, DILATED_M3D, k = 3,                      |
    |           |                    | m3d_conv3d_wgrad_narrow_dilated_f16x2_supported at dilation 2, work >= it                      |
    |           | WGRAD_DILATED      | dilation 2 otherwise                                                                           |
    |           | WGRAD_NARROW_F16X2 | setting.wgrad_narrow_f16 is a threshold, k = 3, m3d_conv3d_wgrad_narrow_f16x2_supported,       |
    |           |                    | work >= it                                                                                     |
    |           | else               | wgrad_kernel(...) under setting.wgrad / wgrad_narrow                                           |
    | gy_reduce | True               | dilation 1 and: train is f16x2 and (dgrad or wgrad is f16x2, or gb needed); or dgrad is narrow |
    |           | True               | dilation 2 and dgrad is TRAIN_DILATED_F16X2                                                    |
    | gb        | None               | gb not needed                                                                                  |
    |           | GB_REDUCE          | gy_reduce                                                                                      |
    |           | GB_BIAS_GRAD       | else                                                                                           |

    compat asks the two halves when it needs them (plan_train_forward in forward, plan_train_backward in backward): a call makes the
    library queries of the directions it runs and no others."""
    return TrainConvPlan(*(plan_train_forward(setting, xshape, wshape, dilation)
                           + plan_train_backward(setting, xshape, wshape, dilation, needs)))


def plan_conv(layer, shape, argmax=False, f16=True, winograd=True, narrow_f16=False):
    """The kernel for `layer` (a LayerConv: cin, cout, k, pool and the packs the switches M3D_WINO / M3D_CONV_F16 gave it) on an input
    [B, cin, D, H, W], shape = (B, D, H, W).  Host queries of the library only.  The caller's needs:
    argmax    PRM mode: a pooled layer must deliver the pool's arg-max.  Only the direct kernels (fused, or ops.maxpool3d_2x behind the
              conv) and the 2-D Winograd family's fused pool do: such a layer never runs on f16x2, on un-fused Winograd or on the F(2,5) stem
    f16       the f16x2 kernel may run this layer (the PRM forward keeps the RPN conv off it)
    winograd  False: direct kernels only (PRMEngine(wino_forward=False))
    narrow_f16  the narrow f16x2 kernel may run this layer (opt-in: the conv box head under M3D_HEAD_CONV_F16): a k = 3 layer without
              pool whose map ZwConv3d does not take, that ZnConv3d (layer.zn) takes and whose launch has at least ZN_MIN_UNITS units is ZN"""
    B, D, H, W = (int(v) for v in shape)
    pool = layer.pool
    zn = getattr(layer, "zn", None)
    if (narrow_f16 and zn is not None and layer.k == 3 and not pool and not (layer.zw is not None and layer.zw.supports((D, H, W)))
            and zn.supports((D, H, W)) and zn.units((B, layer.cin, D, H, W)) >= ZN_MIN_UNITS):
        return Plan(ZN, False, True)
    if winograd and layer.cin * D * H * W * 4 < ITEM_LIMIT:
        if layer.stem is not None and not argmax and layer.stem.supports(W):
            return Plan(STEM, pool, False)
        zw, wino = layer.zw, layer.wino
        if zw is not None and f16 and not (argmax and pool) and zw.supports((D, H, W)) and zw.units((B, layer.cin, D, H, W)) >= ZW_MIN_UNITS:
            return Plan(ZW, pool and zw.supports((D, H, W), pool=True), True)
        if wino is not None and (not (argmax and pool) or (wino.two_d and wino.supports_pool(W))) and wino.supports(W, (B, D, H, W)):
            return Plan(layer.wino_kind, pool and wino.supports_pool(W), False)
    # conv + BN + ReLU + MaxPool in one direct kernel where its 32 x 4 x 4 tile still fills the chip
    return Plan(DIRECT, pool and layer.conv.supports_pool(W, B * D * H * W), False)


class LayerConv:
    """One conv (+ eval-BN scale / shift + ReLU [+ MaxPool3d(2,2)]) layer: its weight packs - direct always; Winograd (3^3: F(2x2,3x3) /
    F(2x4,3x3) on (y,x), 4/9 or 1/3 of the MFMA work, wino_mode 2; F(2,3) along x, 2/3, wino_mode 1), the F(2,5)-along-x stem (5^3, one
    input channel) and f16x2 F(2,3)z (cin % 16 == 0, conv_f16) where the switches allow them - and the execution of a plan.
    The only writer of the tensor attribute `_m3d_bound` (read by DetectorM3D._bound)."""

    def __init__(self, weight, scale, shift, pool, wino_mode, conv_f16, narrow_f16=False):
        self.cout, self.cin, self.k = int(weight.shape[0]), int(weight.shape[1]), int(weight.shape[-1])
        self.scale, self.shift, self.pool, self.conv_f16 = scale, shift, bool(pool), bool(conv_f16)
        self.conv = ops.PackedConv3d(weight)
        self.wino = ops.WinoConv3d(weight, two_d=(wino_mode == 2)) if (wino_mode and self.k == 3) else None
        self.stem = ops.StemWinoConv3d(weight) if (wino_mode and tuple(weight.shape[1:]) == (1, 5, 5, 5)) else None
        self.zw = ops.ZwConv3d(weight) if (conv_f16 and ops.ZwConv3d.supported(weight)) else None
        # the narrow-map f16x2 pack (maps at most 8 wide: the per-RoI convs), only where the caller asked for it
        self.narrow_f16 = bool(narrow_f16 and conv_f16)
        self.zn = ops.ZnConv3d(weight) if (self.narrow_f16 and not pool and ops.ZnConv3d.supported(weight)) else None
        self.wino_kind = None if self.wino is None else "winograd F(2,3)x" if wino_mode != 2 else \
            "winograd F(2x4,3x3)" if ops.lib().m3d_conv3d_wino2_family() == 4 else "winograd F(2x2,3x3)"
        self._plans = {}

    def plan(self, shape, argmax=False, f16=True, winograd=True):
        """plan_conv, asked once per input shape and set of needs (a running pipeline pays no library query per layer per step)"""
        key = (tuple(int(v) for v in shape), argmax, f16, winograd)
        p = self._plans.get(key)
        if p is None:
            p = self._plans[key] = plan_conv(self, *key, narrow_f16=self.narrow_f16) if self.narrow_f16 else plan_conv(self, *key)
        return p

    def __call__(self, x, bound_of, out_max=None, argmax=False, **needs):
        """The layer on x, on the kernel plan_conv picks for the caller's needs -> y, or (y, pool arg-max or None) with argmax.
        bound_of(x): x's operand bound, asked where the plan says sweep (DetectorM3D._bound).  out_max: a ZEROED [ZwConv3d.SLOTS] tensor
        for y's bound (None: a fresh one; False: nobody needs it); y carries the bound it got as `_m3d_bound`."""
        p = self.plan((x.shape[0],) + tuple(x.shape[2:]), argmax=argmax, **needs)
        kw = dict(scale=self.scale, shift=self.shift, relu=True)
        want_am = dict(return_argmax=True) if argmax else {}
        in_max = bound_of(x) if p.sweep else None
        bound = None
        if p.kind == STEM:
            if self.conv_f16:
                bound = out_max if out_max is not None else torch.zeros((ops.ZwConv3d.SLOTS,), dtype=torch.float32, device=x.device)
            y = (self.stem.pooled if p.fused else self.stem)(x, bound=bound if bound is not None else False, **kw)
        elif p.kind == ZW:
            y, bound = self.zw(x, in_max, pool=p.fused, out_max=out_max, **kw)
        elif p.kind == ZN:
            y, bound = self.zn(x, in_max, out_max=out_max, **kw)
        elif p.kind == DIRECT:
            y = self.conv.pooled(x, **kw, **want_am) if p.fused else self.conv(x, **kw)
        else:
            y = self.wino.pooled(x, **kw, **want_am) if p.fused else self.wino(x, **kw)
        if self.pool and not p.fused:
            y = ops.maxpool3d_2x(y, **want_am)
        y, am = y if (argmax and self.pool) else (y, None)
        if bound is not None:
            # valid for this version of y.  A fused pool's epilogue takes the maximum over the pooled values; behind an un-fused pool the
            # bound is the un-pooled map's, which bounds the pooled map too
            y._m3d_bound = (bound, y._version)
        return (y, am) if argmax else y
