"""The accuracy contract of the up-conv's f16x2 backward (csrc/upconv3d_bwd_f16.hip), its cases and their fp64 references (no GPU needed).

    g = gy where y > 0 (y None: g = gy)          n = 8 co + 4 a + 2 b + c          col = (r, z, y, x)
    dgrad  gx[col, ci] = sum_n g[col, n] W[ci, n]        wgrad  gW[ci, n] = sum_col x[col, ci] g[col, n]        gb[co] = sum g

Per element the formula of f16x2_contract.bound (derived in that module's docstring), as tests/linear_backward_f16_cases.py states it:
  * c1 = 3.01: neither operand is rounded before the cut (both are the raw fp32 tensors; the mask is a select, not an operation);
  * A = max|gy| of the UNMASKED gy (the bound the kernel scales g with), B = max|W| (dgrad) / max|x| (wgrad);
  * n_acc = chain * max(folds, 1) + folds + slices + 2 from the library's _plan calls (one rounding per MFMA of a chain, one per fold,
    one per slice the reduce launch adds, the two scale multiplies).
gb is summed from the uncut fp32 values: upconv_reference.bound with n = 8 R D H W + gb_partials.  Where C == 0 the bound is 0: the
output is exactly 0 (a dead channel's gW and gb).

The cases (R, Cin, Cout, D, H, W) are the smallest shapes at which each mechanism can go wrong (dgrad: 64 columns per workgroup, chunks
of 4 output channels; wgrad: tiles of 128 x 128, chunks of 32 columns, at most 16 slices, a fold every 64 chunks)."""
import functools

import numpy as np
import torch

import f16x2_contract as FC
import upconv_reference as UR
from linear_backward_f16_cases import C1, MAX_CHAIN, bound, n_acc, violations, worst_ratio  # noqa: F401  (the same contract formula)

F64 = torch.float64
CASES = {
    "one": (1, 32, 32, 1, 1, 1),          # one voxel: the wgrad's K is a single column against a 16-deep step
    "ragged": (3, 32, 64, 2, 3, 5),       # odd extents, 30 columns per RoI, a column tile spanning RoIs, Cout != Cin
    "roi_grid": (2, 64, 32, 7, 7, 7),     # V = 343: no row is a 16-byte multiple
    "wide_row": (2, 32, 32, 3, 4, 33),    # a row longer than a tile
    "shipped": (1, 256, 256, 7, 7, 7),    # the real channel counts, one RoI
    "deep": (2, 32, 288, 2, 2, 2),        # dgrad K = 2304 -> 432 MFMAs > 384: the dgrad plan reports folds >= 1
    # 5488 columns make 172 chunks, which this kernel cuts into 16 slices of 11: no fold.  R raised from 16 to 96: 32 928 columns =
    # 1029 chunks = 16 slices of 65 chunks, one more than a chain holds - the wgrad plan reports slices >= 2 AND folds >= 1
    "split": (96, 32, 32, 7, 7, 7),
    "walk": (97, 32, 32, 7, 7, 7),        # 520 dgrad column tiles: more than the 512 resident workgroup slots, the last one ragged
}
FAMILIES = ("benign", "heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below", "relu_mask", "dead_channel")
MUTANTS = ("hi_only", "drop_hilo", "lo_unscaled")
DEAD = 1                                   # the output channel whose y <= 0 everywhere in the dead_channel family


def to_cols(g):
    """[R,Co,2D,2H,2W] -> G [R D H W, 8 Co] with G[(r,z,y,x), 8 co + 4a + 2b + c] = g[r,co,2z+a,2y+b,2x+c]"""
    R, Co, D2, H2, W2 = g.shape
    return g.reshape(R, Co, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, 8 * Co)


def to_cols_swapped(g):
    """to_cols with the parities b and c exchanged (the `swap_bc` mutant)"""
    R, Co, D2, H2, W2 = g.shape
    return g.reshape(R, Co, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2).permute(0, 2, 4, 6, 1, 3, 7, 5).reshape(-1, 8 * Co)


def dgrad_op(g, w, cols=to_cols):
    """g [R,Co,2D,2H,2W] (masked), w [Ci,Co,2,2,2] -> gx [R,Ci,D,H,W]; bilinear"""
    R, _, D2, H2, W2 = g.shape
    out = cols(g) @ w.reshape(w.shape[0], -1).T
    return out.reshape(R, D2 // 2, H2 // 2, W2 // 2, -1).permute(0, 4, 1, 2, 3)


def wgrad_op(g, x, cols=to_cols):
    """g [R,Co,2D,2H,2W] (masked), x [R,Ci,D,H,W] -> gW [Ci,Co,2,2,2]; bilinear"""
    X = x.permute(0, 2, 3, 4, 1).reshape(-1, x.shape[1])
    return (X.T @ cols(g)).reshape(x.shape[1], g.shape[1], 2, 2, 2)


OPS = {"dgrad": dgrad_op, "wgrad": wgrad_op}


def mask_of(gy, y):
    """g: gy where y > 0 (a select), gy itself without y"""
    return gy if y is None else torch.where(y > 0, gy, torch.zeros_like(gy))


def make_inputs(name, kind):
    """gy [R,Cout,2D,2H,2W] (the family's input, signed), w [Cin,Cout,2,2,2], x [R,Cin,D,H,W] (its weights, two draws) and y (the
    forward's output: random, about half <= 0; in dead_channel channel DEAD is <= 0 everywhere), fp32"""
    R, Cin, Cout, D, H, W = CASES[name]
    seed = R + 7 * Cin + 13 * Cout + 17 * D + 19 * H + 23 * W
    fam = "benign" if kind in ("relu_mask", "dead_channel") else kind
    gshape = (R, Cout, 2 * D, 2 * H, 2 * W)
    gy, w = FC.inputs(fam, gshape, (Cin, Cout, 2, 2, 2), seed, True)
    _, x = FC.inputs(fam, gshape, (R, Cin, D, H, W), seed + 1, True)
    y = torch.randn(gshape, generator=torch.Generator().manual_seed(seed + 2))
    if kind == "dead_channel":
        y[:, DEAD] = -y[:, DEAD].abs()
    f = lambda t: t.to(torch.float32).contiguous()
    return f(gy), f(w), f(x), f(y)


def build(shape, gy, w, x, y):
    """The tensor maxima, fp64 references and bound terms of one set of fp32 CPU inputs (y None: no mask)"""
    g = mask_of(gy, y)
    out = dict(shape=tuple(shape), gy=gy, w=w, x=x, y=y, g=g, A=float(gy.abs().max()),
               B=dict(dgrad=float(w.abs().max()), wgrad=float(x.abs().max())))
    for d, b in (("dgrad", w), ("wgrad", x)):
        out[d] = (OPS[d](g.to(F64), b.to(F64)),) + FC.terms(OPS[d], g, b)
    g64 = g.to(F64)
    out["gb"] = (g64.sum(dim=(0, 2, 3, 4)), g64.abs().sum(dim=(0, 2, 3, 4)))
    return out


@functools.lru_cache(maxsize=2)
def case(name, kind, masked):
    """`build` of the inputs of one case, computed once and shared (treat as read-only).  masked: the ReLU mask y is applied
    (out["y"], else None)"""
    gy, w, x, y = make_inputs(name, kind)
    return build(CASES[name], gy, w, x, y if masked else None)


def contract(c, direction, nacc, A=None, B=None):
    """(fp64 reference, E, C) of a direction of a case at the given n_acc; A, B: the bounds the kernel was given (None: the maxima)"""
    y, C, Sa, Sb, n = c[direction]
    return y, bound(C, Sa, Sb, n, c["A"] if A is None else A, c["B"][direction] if B is None else B, y, nacc), C


def gb_contract(c, gb_partials):
    """(fp64 reference, E) of the bias gradient: fp32 sums of 8 R D H W terms and gb_partials partial sums"""
    R, _, _, D, H, W = c["shape"]
    ref, A = c["gb"]
    return ref, torch.from_numpy(np.asarray(UR.bound(ref.numpy(), A.numpy(), 8 * R * D * H * W + gb_partials)))


def emulate(c, direction, mutant=None):
    """the direction as the kernel computes it, summed exactly (f16x2_contract.emulate).  mutant: those of f16x2_contract.emulate, or
    "swap_bc" (the parities b and c of gy exchanged), "no_mask" (the ReLU mask dropped)"""
    b = c["w"] if direction == "dgrad" else c["x"]
    op, g = OPS[direction], c["g"]
    if mutant == "swap_bc":
        op, mutant = functools.partial(OPS[direction], cols=to_cols_swapped), None
    elif mutant == "no_mask":
        g, mutant = c["gy"], None
    return FC.emulate(op, g, b, c["A"], c["B"][direction], mutant)
