"""The cases of the narrow-map f16x2 conv at DILATION 2 (csrc/conv3d_zn.hip, conv3d_zn_kernel<2>; ops.ZnConv3d(..., dilation=2)): a 3^3
stride-1 conv with dilation 2 and padding 2 on maps at most 8 wide, forward and backward-data, with fp64 references and the per-element
bound of tests/f16x2_contract.py.  No GPU needed.

  forward   y = conv3d(x, w, padding=2, dilation=2) scale + shift [ReLU]
  dgrad     gx = conv_transpose3d(gy, w_forward, padding=2, dilation=2)     the same kernel on the pack of w.flip(2, 3, 4).transpose(0, 1)

The arithmetic is the dilation-1 kernel's line for line (the same cut at staging, three MFMAs per product, fp32 accumulation, one
multiply and one add in the epilogue), so the constants of tests/conv_f16_narrow_cases.py carry over unchanged: c1 = 3.01,
n_acc = 81 cin / 16 + 1, and with them bound_E, the input families, integer_inputs, finish, cut, emulate and terms.  What differs is the
geometry: a tap reads at 2 (d - 1), the halo is 2 voxels per side.  The cases are the dilation-1 table's shapes, several of which mean
something new here, and one more:
  cout5    D = 2: every dz != 1 tap reads outside the volume - exactly zero
  tiles    the 2-voxel halo crosses the y (8) and z (4) tile edges on both sides
  w3       dx = +-2 connects only x = 0 and x = 2
  w2       every dx != 1 tap is exactly zero
  ragged_walk   the batch comes from the library's own unit count (m3d_conv3d_zn_dilated_launch_units): 256 units + a ragged remainder"""
import torch

import conv_f16_narrow_cases as T
from f16x2_contract import cut, emulate, terms            # noqa: F401  (re-exported for the tests)

F64 = torch.float64
Fn = torch.nn.functional
C1, n_acc, bound_E = T.C1, T.n_acc, T.bound_E
FAMILIES, DIRECTIONS, CUT_MUTANTS = T.FAMILIES, T.DIRECTIONS, T.CUT_MUTANTS
integer_inputs_of, finish, dgrad_weight, forward_weight, bounds = T.integer_inputs, T.finish, T.dgrad_weight, T.forward_weight, T.bounds
DILATION = 2
TILE_Y, TILE_Z = 8, 4                         # the kernel's voxel tile (x: the whole row)

RAGGED = (16, 8, 7, 7, 7)                     # (cin, cout, D, H, W) of ragged_walk


def ragged_batch():
    """the batch of ragged_walk: the smallest whose launch has 256 units and a ragged remainder of 6 more, by the library's own count"""
    from m3d._lib import lib
    cin, cout, D, H, W = RAGGED
    per_item = int(lib().m3d_conv3d_zn_dilated_launch_units(1, cin, cout, D, H, W, DILATION))
    assert per_item >= 1
    return (T.CUS + 6 + per_item - 1) // per_item


_cases = None


def cases():
    """name -> (B, cin, cout, D, H, W) of the conv that is LAUNCHED: the eight shapes of the dilation-1 table (ragged_walk's batch from the
    library) and w2"""
    global _cases
    if _cases is None:
        c = {k: v for k, v in T.CASES.items() if k != "ragged_walk"}
        c["ragged_walk"] = (ragged_batch(),) + RAGGED
        c["w2"] = (1, 16, 32, 5, 6, 2)
        _cases = c
    return _cases


CASE_NAMES = tuple(sorted(set(T.CASES) | {"w2"}))
GEOMETRY_DEFECTS = ("drop_tap", "halo_z", "halo_y", "halo_x", "halo_1", "clamp_pad", "dilation_1_taps")


def conv_op(x, w):
    """the dilated 'same' conv, bilinear in (x, w)"""
    return Fn.conv3d(x, w, padding=DILATION, dilation=DILATION)


def _halo_1(x, w):
    """the conv as a kernel whose halo tile holds ONE voxel per side computes it: a tap that reads two voxels beyond its output's
    8 (y) x 4 (z) tile finds zero (x: the tile is the whole row, beyond it lies only padding)"""
    D, H = x.shape[2], x.shape[3]
    z, y = torch.arange(D), torch.arange(H)
    out = 0
    for dz in range(3):
        rz = z + DILATION * (dz - 1)
        mz = ((rz >= (z // TILE_Z) * TILE_Z - 1) & (rz <= (z // TILE_Z) * TILE_Z + TILE_Z)).to(x.dtype).view(1, 1, D, 1, 1)
        for dy in range(3):
            ry = y + DILATION * (dy - 1)
            my = ((ry >= (y // TILE_Y) * TILE_Y - 1) & (ry <= (y // TILE_Y) * TILE_Y + TILE_Y)).to(x.dtype).view(1, 1, 1, H, 1)
            wt = torch.zeros_like(w)
            wt[:, :, dz, dy, :] = w[:, :, dz, dy, :]
            out = out + conv_op(x, wt) * mz * my
    return out


def defect_op(name):
    """conv_op with a seeded geometry defect (bilinear in (x, w), so `emulate` takes it): a dropped tap; a halo origin off by one along
    an axis (the tile read one voxel early); a halo of one voxel; edge clamp instead of zero padding; the tap offsets of dilation 1"""
    def op(x, w):
        if name == "drop_tap":
            w = w.clone()
            w[:, :, 1, 0, 1] = 0                  # (dz = dx = 1: a tap that D = 1, D = 2 and W = 2 leave inside the map)
            return conv_op(x, w)
        if name == "halo_1":
            return _halo_1(x, w)
        if name == "clamp_pad":
            return Fn.conv3d(Fn.pad(x, (2,) * 6, mode="replicate"), w, dilation=DILATION)
        if name == "dilation_1_taps":
            return Fn.conv3d(x, w, padding=1)
        pad = {"halo_x": (3, 1, 2, 2, 2, 2), "halo_y": (2, 2, 3, 1, 2, 2), "halo_z": (2, 2, 2, 2, 3, 1)}[name]
        return Fn.conv3d(Fn.pad(x, pad), w, dilation=DILATION)
    return op


def make(case, direction, family, seed=5):
    """(a, wl, scale, shift, relu) as conv_f16_narrow_cases.make, on this table's shapes"""
    B, cin, cout, D, H, W = cases()[case]
    a, wl = T.inputs(family, (B, cin, D, H, W), (cout, cin, 3, 3, 3), seed, signed=(direction == "dgrad"))
    if direction == "dgrad":
        return a, wl, None, None, False
    g = torch.Generator().manual_seed(seed + 1)
    return a, wl, torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g), True


def integer_inputs(case, direction, seed=3):
    """x, w in [-3, 3], integer shift (conv_f16_narrow_cases.integer_inputs: exact in the kernel, whatever the dilation)"""
    B, cin, cout, D, H, W = cases()[case]
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (B, cin, D, H, W), generator=g).float()
    wl = torch.randint(-3, 4, (cout, cin, 3, 3, 3), generator=g).float()
    shift = torch.randint(-5, 6, (cout,), generator=g).float() if direction == "forward" else None
    return a, wl, shift


def reference_op(direction, a, wl, scale=None, shift=None, relu=False):
    """fp64: F.conv3d(x, w, padding=2, dilation=2) scale + shift [ReLU]; a dgrad is conv_transpose3d on the FORWARD parameter"""
    if direction == "forward":
        return finish(conv_op(a.to(F64), wl.to(F64)), scale, shift, relu)
    return Fn.conv_transpose3d(a.to(F64), dgrad_weight(wl).to(F64), padding=DILATION, dilation=DILATION)


def contract(direction, a, wl, scale=None, shift=None, relu=False, in_bound=None):
    """(fp64 reference, E, C) of the launched conv with operand bound in_bound (None: max|a|)"""
    A, B = bounds(a, wl, in_bound)
    C, Sa, Sb, n = terms(conv_op, a, wl)
    y = reference_op(direction, a, wl, scale, shift, relu)
    gain = 1.0 if scale is None else scale.to(F64).abs().view(1, -1, 1, 1, 1)
    return y, bound_E(a.shape[1], C, Sa, Sb, n, A, B, y, gain), C


def emulated(a, wl, scale=None, shift=None, relu=False, in_bound=None, mutant=None, defect=None):
    """the kernel's result with exact accumulation (fp64): the three products of the cut operands, then the epilogue"""
    A, B = bounds(a, wl, in_bound)
    return finish(emulate(defect_op(defect) if defect else conv_op, a, wl, A, B, mutant), scale, shift, relu)


_cache = {}


def reference(case, direction, family):
    """(a, wl, scale, shift, relu, y, E, C), computed once and shared (never modified)"""
    key = (case, direction, family)
    if key not in _cache:
        a, wl, scale, shift, relu = make(case, direction, family)
        _cache[key] = (a, wl, scale, shift, relu) + tuple(contract(direction, a, wl, scale, shift, relu))
    return _cache[key]
