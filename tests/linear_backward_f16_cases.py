"""The accuracy contract of the f16x2 linear backward (csrc/fc_backward_f16.hip), its cases and their fp64 references (no GPU needed).

    dgrad  gx[M,K] = gy[M,N] . W[N,K]        wgrad  gw[N,K] = gy[M,N]^T . x[M,K]        gb[N] = sum_m gy[m,n]

Per element the formula of f16x2_contract.bound (derived in that module's docstring) with
  * c1 = 3.01: neither operand is rounded before the cut (both are the raw fp32 tensors);
  * A, B = the two tensor maxima (one scale per operand tensor): max|gy| and max|W| (dgrad) / max|x| (wgrad);
  * n_acc from what the library's _plan function reports, derived from the code: an output's running sum is rounded once per MFMA of
    its chain (at most `chain` between two folds, so at most chain * max(folds, 1) in a slice), once per fold into the fp32 registers,
    once per slice added by the reduce launch, and the two scale multiplies: n_acc = chain * max(folds, 1) + folds + slices + 2.
gb is summed from the uncut fp32 values: it stays within linear_backward_reference.bias_bound.  Where C == 0 the bound is 0: the output
is exactly 0.

The cases (M, N, K) are the smallest shapes at which each mechanism can go wrong (the tile is 128 x 128, the reduction chunk 32, the
MFMA step 16): (1,64,32) one row; (36,64,128) M ragged against the 16-deep step; (77,96,160) every dimension ragged against its tile;
(129,192,2752) a second row tile holding one row, two N tiles; (33,1024,1024) fc2: split reduction; (260,128,4096) M > 256;
(64,64,1152) nine column tiles; (40,2112,64) dgrad chain beyond 384: folds; (2100,64,64) wgrad chain beyond 384.
The families are those of f16x2_contract.inputs applied to gy (signed), and the zero_rows kind of linear_backward_reference."""
import functools

import torch

import f16x2_contract as FC
import linear_backward_reference as R

F64 = torch.float64
C1 = 3.01
CASES = [(1, 64, 32), (36, 64, 128), (77, 96, 160), (129, 192, 2752), (33, 1024, 1024), (260, 128, 4096), (64, 64, 1152), (40, 2112, 64),
         (2100, 64, 64)]
FAMILIES = ("benign", "heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below", "zero")
KINDS = FAMILIES + ("zero_rows",)
MUTANTS = ("hi_only", "drop_hilo", "lo_unscaled", "scale_up")
MAX_CHAIN = 384


def dgrad_op(gy, w):
    return gy @ w


def wgrad_op(gy, x):
    return gy.T @ x


OPS = {"dgrad": dgrad_op, "wgrad": wgrad_op}


def make_inputs(M, N, K, kind):
    """gy [M,N], w [N,K], x [M,K] fp32: gy is the family's input, w and x its weights (two draws)"""
    seed = M + 7 * N + 13 * K
    name = "benign" if kind == "zero_rows" else kind
    gy, w = FC.inputs(name, (M, N), (N, K), seed, True)
    _, x = FC.inputs(name, (M, N), (M, K), seed + 1, True)
    gy, w, x = gy.to(torch.float32).contiguous(), w.to(torch.float32).contiguous(), x.to(torch.float32).contiguous()
    if kind == "zero_rows":
        gy[1::3] = 0.0
    return gy, w, x


def n_acc(plan):
    """roundings of an output's running sum, from dict(slices, chain, folds) of the library's _plan function"""
    return plan["chain"] * max(plan["folds"], 1) + plan["folds"] + plan["slices"] + 2


def bound(C, Sa, Sb, n, A, B, y, nacc):
    """f16x2_contract.bound with c1 = C1 and the given n_acc"""
    F = FC.C2 * 2.0 ** -39 * (A * Sb + B * Sa) + 2.0 ** -77 * n * A * B
    return C1 * 2.0 ** -22 * C + F + FC.C3 * nacc * 2.0 ** -24 * (C + F) + 2.0 ** -24 * y.abs()


@functools.lru_cache(maxsize=None)
def case(M, N, K, kind):
    """The inputs, tensor maxima, fp64 references and bound terms of one case, computed once and shared (treat as read-only)"""
    gy, w, x = make_inputs(M, N, K, kind)
    out = dict(gy=gy, w=w, x=x, A=float(gy.abs().max()), B=dict(dgrad=float(w.abs().max()), wgrad=float(x.abs().max())))
    for name, b in (("dgrad", w), ("wgrad", x)):
        op = OPS[name]
        out[name] = (op(gy.to(F64), b.to(F64)),) + FC.terms(op, gy, b)
    out["bias"] = R.bias_bound(gy.numpy())
    return out


def contract(c, name, nacc):
    """(fp64 reference, E, C) of op `name` of a case at the given n_acc"""
    y, C, Sa, Sb, n = c[name]
    return y, bound(C, Sa, Sb, n, c["A"], c["B"][name], y, nacc), C


def emulate(c, name, mutant=None):
    """the op as the kernel computes it, summed exactly (f16x2_contract.emulate)"""
    b = c["w"] if name == "dgrad" else c["x"]
    return FC.emulate(OPS[name], c["gy"], b, c["A"], c["B"][name], mutant)


def violations(got, y, E):
    """elements outside the bound; a non-finite value counts"""
    return int((~((got.to(F64) - y).abs() <= E)).sum())


def worst_ratio(got, y, E):
    """largest |got - y| / E; an element with E == 0 counts 0 when it is exactly right and inf when it is not"""
    err = (got.to(F64) - y).abs()
    r = torch.where(E > 0, err / E, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0
