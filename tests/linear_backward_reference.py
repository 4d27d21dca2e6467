"""Reference and per-element error bound for the box head's linear backward (csrc/fc_backward.hip):

    dgrad  gx[M,K] = gy[M,N] . W[N,K]        wgrad  gw[N,K] = gy[M,N]^T . x[M,K]        gb[N] = sum_m gy[m,n]

The bound is derived, not fitted.  The fp32-input MFMA is a chain of fused multiply-adds, so an output summed over R terms whose S split
partials are added afterwards carries at most n = R + S roundings, and for ANY summation order (Higham, Accuracy and Stability of
Numerical Algorithms, 3.1: the bound does not depend on the order, and a rounded product followed by a rounded sum satisfies it as well)

    |out - out64| <= gamma_n sum_k |a_k b_k| + 2^-24 |out64|,      gamma_n = n u / (1 - n u),  u = 2^-24

with both sums taken in fp64 from the fp32 inputs (a product of two fp32 numbers is exact in fp64; the fp64 sum's own error is 2^-29 of
the fp32 one).  The last term is the final rounding of an exactly accumulated value, which keeps the bound valid for the identity cases
(R = 1).  S is not read from the code under test: the contract allows at most 64 slices, so S = 64 everywhere.  gb adds M numbers, which
takes M - 1 additions however the sum is cut, so n = M.  Where sum |a b| = 0 the bound is 0: the output must be exactly 0."""
import functools

import numpy as np

U = 2.0 ** -24
MAX_SLICES = 64

# (M, N, K): see tests/test_gpu_linear_backward.py for what each one is for
CASES = [(1, 2, 8), (36, 64, 128), (77, 2, 1024), (77, 12, 1024), (128, 256, 2744), (129, 130, 2744), (33, 1024, 1024), (260, 128, 4096)]
KINDS = ("randn", "zero_rows", "small")


def gamma(n):
    return n * U / (1.0 - n * U)


def make_inputs(M, N, K, kind, seed=0):
    """gy [M,N], w [N,K], x [M,K] fp32.  kind: 'randn'; 'zero_rows': every row m of gy with m % 3 == 1 is zero (the padding rows of
    box_head_losses); 'small': gy scaled by 2^-20, the magnitude of a gradient."""
    rng = np.random.RandomState(1000 * seed + M + 7 * N + 13 * K)
    gy = rng.standard_normal((M, N)).astype(np.float32)
    w = rng.standard_normal((N, K)).astype(np.float32)
    x = rng.standard_normal((M, K)).astype(np.float32)
    if kind == "zero_rows":
        gy[1::3] = 0.0
    elif kind == "small":
        gy *= np.float32(2.0 ** -20)
    elif kind != "randn":
        raise ValueError(kind)
    return gy, w, x


def _bound(a64, b64, n):
    ref = a64 @ b64
    mag = np.abs(a64) @ np.abs(b64)
    return ref, gamma(n) * mag + U * np.abs(ref)


def dgrad_bound(gy, w, slices=MAX_SLICES):
    """(ref64 [M,K], E [M,K])"""
    return _bound(gy.astype(np.float64), w.astype(np.float64), gy.shape[1] + slices)


def wgrad_bound(gy, x, slices=MAX_SLICES):
    """(ref64 [N,K], E [N,K])"""
    return _bound(gy.astype(np.float64).T, x.astype(np.float64), gy.shape[0] + slices)


def bias_bound(gy):
    """(ref64 [N], E [N])"""
    g = gy.astype(np.float64)
    ref = g.sum(0)
    return ref, gamma(gy.shape[0]) * np.abs(g).sum(0) + U * np.abs(ref)


@functools.lru_cache(maxsize=None)
def case(M, N, K, kind):
    """The inputs and the three (ref64, E) pairs of one case, computed once and shared (read-only) by every test that needs them."""
    gy, w, x = make_inputs(M, N, K, kind)
    out = dict(gy=gy, w=w, x=x, dgrad=dgrad_bound(gy, w), wgrad=wgrad_bound(gy, x), bias=bias_bound(gy))
    for v in (gy, w, x) + out["dgrad"] + out["wgrad"] + out["bias"]:
        v.setflags(write=False)
    return out


def worst_ratio(got, ref, E):
    """largest |got - ref| / E; an element with E == 0 counts 0 when it is exactly right and inf when it is not"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(E > 0, err / E, np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def sequential_f32(a, b):
    """a [R,P]^T-free form: out[p,q] = sum_r a[r,p] b[r,q] accumulated one r at a time in fp32 (rounded product, rounded sum)"""
    acc = np.zeros((a.shape[1], b.shape[1]), dtype=np.float32)
    for r in range(a.shape[0]):
        acc += a[r][:, None] * b[r][None, :]
    return acc


def to_bf16(a):
    """fp32 -> bf16 (round to nearest even) -> fp32"""
    bits = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(np.float32).reshape(a.shape)
