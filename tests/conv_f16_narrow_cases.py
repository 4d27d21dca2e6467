"""The cases of the narrow-map f16x2 conv (csrc/conv3d_zn.hip, ops.ZnConv3d): a 3^3 stride-1 pad-1 conv on maps at most 8 wide, forward
and backward-data, with fp64 references and the per-element bound of tests/f16x2_contract.py.  No GPU needed.

  forward   y = conv3d(x, w) scale + shift [ReLU]            operands a = x (bound A = in_max), b = w (bound B = fl(max|w|))
  dgrad     gx = conv_transpose3d(gy, w)                     the same kernel on the pack of w.flip(2, 3, 4).transpose(0, 1)

The kernel's constants, from its code (not from a fit):
  c1 = 3 + 2^-22 (written 3.01): the DIRECT form cuts x and w themselves - neither operand is rounded to fp32 before the cut (the zw
      kernel's 0.5 is the fp32 rounding of its Winograd operands V_k and U_k, which this kernel does not form);
  n_acc = 81 cin / 16 + 1: one workgroup holds the whole K, so an accumulator sees 27 taps x cin / 16 chunks x 3 MFMAs, and the epilogue
      applies ONE fp32 operation before its last one: the multiply by scale[c] / (s_a s_b) (the power of two is folded into the scale
      exactly); the last operation is the shift add, whose rounding is the bound's 2^-24 |y| term.  No split-K partial sums, no
      Winograd combination.
A zero product is exact (the cut of 0 is 0), so where C == 0 the output is exactly the shift."""
import torch

from f16x2_contract import cut, emulate, terms, conv3d_op, inputs, C2, C3            # noqa: F401  (cut: re-exported for the tests)

F64 = torch.float64
C1 = 3.01


def n_acc(cin):
    return 81 * cin / 16 + 1


# (B, cin, cout, D, H, W) of the conv that is LAUNCHED (a dgrad case launches it on the dgrad pack of a forward weight [cin, cout, ...])
CUS = 256                                     # compute units of the chip: the ragged-walk case is stated against it
CASES = {
    "roi_grid": (3, 32, 64, 7, 7, 7),         # the RoI grid: 7 of 8 along x and y, a partial z tile
    "full": (2, 16, 32, 8, 8, 8),             # full tiles, one chunk
    "cout5": (1, 16, 5, 2, 8, 8),             # cout below a block, one unit
    "short": (2, 48, 33, 3, 5, 7),            # three chunks, cout one past a 32-block, all extents short
    "d1": (5, 32, 64, 1, 7, 7),               # D = 1: every dz != 1 tap is exactly zero
    "tiles": (1, 64, 32, 14, 14, 8),          # several y and z tiles
    "w3": (2, 32, 40, 7, 7, 3),               # a very narrow row
    # one workgroup per unit, no persistent walk: the hardware dispatches the units; this case launches CUS + a ragged remainder of them
    # (2 units per item: 131 x 2 = 262 = 256 + 6), so that a second, partial round of workgroups runs; cout = 8 keeps the fp64
    # references of 131 items small
    "ragged_walk": (131, 16, 8, 7, 7, 7),
}
FAMILIES = ("benign", "heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below")
DIRECTIONS = ("forward", "dgrad")
CUT_MUTANTS = ("hi_only", "drop_hilo", "lo_unscaled")          # on every family; "scale_up" overflows fp16 only at_bound_below
GEOMETRY_DEFECTS = ("drop_tap", "halo_z", "halo_y", "halo_x", "clamp_pad")


def dgrad_weight(w):
    """the weight of the backward-data conv as a forward conv: taps flipped, channel roles swapped"""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def forward_weight(direction, wl):
    """the FORWARD layer's parameter whose launched conv has weight wl [cout, cin, 3, 3, 3]: wl itself, or for a dgrad the layer whose
    backward-data conv wl is"""
    return wl if direction == "forward" else dgrad_weight(wl)


def defect_op(name):
    """conv3d_op with a seeded geometry defect (bilinear in (x, w), so `emulate` takes it): a dropped tap, a halo origin off by one along
    an axis (the tile read one voxel early), a missing zero padding (edge clamp instead of zero)"""
    Fn = torch.nn.functional

    def op(x, w):
        if name == "drop_tap":
            w = w.clone()
            w[:, :, 1, 1, 0] = 0                  # (a tap of the middle plane: the D = 1 case has no other)
            return Fn.conv3d(x, w, padding=1)
        if name == "clamp_pad":
            return Fn.conv3d(Fn.pad(x, (1, 1, 1, 1, 1, 1), mode="replicate"), w)
        pad = {"halo_x": (2, 0, 1, 1, 1, 1), "halo_y": (1, 1, 2, 0, 1, 1), "halo_z": (1, 1, 1, 1, 2, 0)}[name]
        return Fn.conv3d(Fn.pad(x, pad), w)
    return op


def make(case, direction, family, seed=5):
    """(a, wl, scale, shift, relu): the operand (x ReLU'd / gy signed), the LAUNCHED conv's weight, and the forward epilogue (scale, shift,
    ReLU on the forward; a bare conv for dgrad)"""
    B, cin, cout, D, H, W = CASES[case]
    a, wl = inputs(family, (B, cin, D, H, W), (cout, cin, 3, 3, 3), seed, signed=(direction == "dgrad"))
    if direction == "dgrad":
        return a, wl, None, None, False
    g = torch.Generator().manual_seed(seed + 1)
    return a, wl, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), True


def integer_inputs(case, direction, seed=3):
    """x, w in [-3, 3], integer shift: the cut of a small integer is exact (3 s < 2^15 has at most two significant bits: h = v, l = 0),
    every product is an integer times s_a s_b and every partial sum stays below 2^24 of that unit (27 cin 9 <= 2^24 for cin <= 2^16), so
    the fp32 accumulation, the exact un-scaling and the integer shift add are all exact: the result equals the fp64 reference bit for bit"""
    B, cin, cout, D, H, W = CASES[case]
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (B, cin, D, H, W), generator=g).float()
    wl = torch.randint(-3, 4, (cout, cin, 3, 3, 3), generator=g).float()
    shift = torch.randint(-5, 6, (cout,), generator=g).float() if direction == "forward" else None
    return a, wl, shift


def finish(acc, scale=None, shift=None, relu=False):
    """the epilogue on an fp64 sum"""
    if scale is not None:
        acc = acc * scale.to(F64).view(1, -1, 1, 1, 1)
    if shift is not None:
        acc = acc + shift.to(F64).view(1, -1, 1, 1, 1)
    return torch.relu(acc) if relu else acc


def reference_op(direction, a, wl, scale=None, shift=None, relu=False):
    """fp64: F.conv3d(x, w, padding=1) scale + shift [ReLU]; a dgrad is conv_transpose3d on the FORWARD parameter"""
    if direction == "forward":
        return finish(conv3d_op(a.to(F64), wl.to(F64)), scale, shift, relu)
    return torch.nn.functional.conv_transpose3d(a.to(F64), dgrad_weight(wl).to(F64), padding=1)


def bounds(a, wl, in_bound=None):
    """(A, B) of the kernel: the input bound the caller gives (default: max|a|, what a sweep gives) and fl(max|w|)"""
    return (float(a.abs().max()) if in_bound is None else float(in_bound)), float(wl.abs().max())


def bound_E(cin, C, Sa, Sb, n, A, B, y, gain=1.0):
    """E of every output: the formula of f16x2_contract.bound with this kernel's (c1, n_acc)"""
    A, B = torch.as_tensor(A, dtype=F64), torch.as_tensor(B, dtype=F64)
    Fq = C2 * 2.0 ** -39 * (A * Sb + B * Sa) + 2.0 ** -77 * n * A * B
    e = C1 * 2.0 ** -22 * C + Fq + C3 * n_acc(cin) * 2.0 ** -24 * (C + Fq)
    return torch.as_tensor(gain, dtype=F64) * e + 2.0 ** -24 * y.abs()


def contract(direction, a, wl, scale=None, shift=None, relu=False, in_bound=None):
    """(fp64 reference, E, C) of the launched conv with operand bound in_bound (None: max|a|)"""
    A, B = bounds(a, wl, in_bound)
    C, Sa, Sb, n = terms(conv3d_op, a, wl)
    y = reference_op(direction, a, wl, scale, shift, relu)
    gain = 1.0 if scale is None else scale.to(F64).abs().view(1, -1, 1, 1, 1)
    return y, bound_E(a.shape[1], C, Sa, Sb, n, A, B, y, gain), C            # (ReLU is 1-Lipschitz)


def emulated(a, wl, scale=None, shift=None, relu=False, in_bound=None, mutant=None, defect=None):
    """the kernel's result with exact accumulation (fp64): the three products of the cut operands, then the epilogue"""
    A, B = bounds(a, wl, in_bound)
    return finish(emulate(defect_op(defect) if defect else conv3d_op, a, wl, A, B, mutant), scale, shift, relu)


_cache = {}


def reference(case, direction, family):
    """(a, wl, scale, shift, relu, y, E, C), computed once and shared (never modified)"""
    key = (case, direction, family)
    if key not in _cache:
        a, wl, scale, shift, relu = make(case, direction, family)
        _cache[key] = (a, wl, scale, shift, relu) + tuple(contract(direction, a, wl, scale, shift, relu))
    return _cache[key]
