"""CPU: the error bound of the linear backward (tests/linear_backward_reference.py) holds for honest fp32 evaluations and rejects broken
ones; the C ABI of m3d_linear_dgrad / m3d_linear_wgrad refuses what it must before any device pointer is followed or anything is
launched, so every call below is safe with made-up pointers (none of them passes the checks with M > 0)."""
import ctypes as C

import numpy as np
import pytest

import linear_backward_reference as R


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


def evaluations(c, fn):
    """dgrad, wgrad, bias evaluated with `fn(a [R,P], b [R,Q]) -> [P,Q]` (sum over the leading index) and a matching column sum"""
    gy, w, x = c["gy"], c["w"], c["x"]
    return fn(np.ascontiguousarray(gy.T), w), fn(gy, x), fn(gy, np.ones((gy.shape[0], 1), np.float32))[:, 0]


def ratios(c, got):
    return [R.worst_ratio(g, *c[k]) for g, k in zip(got, ("dgrad", "wgrad", "bias"))]


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("M,N,K", R.CASES)
def test_the_bound_holds_for_fp32_evaluations(M, N, K, kind):
    c = R.case(M, N, K, kind)
    for name, fn in (("sequential", R.sequential_f32), ("matmul", lambda a, b: np.matmul(a.T, b))):
        r = ratios(c, evaluations(c, fn))
        print("%s (%d,%d,%d) %s: error / E  dgrad %.3f  wgrad %.3f  bias %.3f" % (name, M, N, K, kind, *r))
        assert max(r) <= 1.0, (name, r)


@pytest.mark.parametrize("kind", ("randn", "small"))
@pytest.mark.parametrize("M,N,K", R.CASES)
def test_the_bound_has_teeth(M, N, K, kind):
    c = R.case(M, N, K, kind)
    gy, w, x = c["gy"], c["w"], c["x"]
    # one operand rounded to bf16
    gyb = R.to_bf16(gy)
    got = (np.matmul(gyb, w), np.matmul(gyb.T, x), gyb.sum(0, dtype=np.float32))
    r = ratios(c, got)
    assert min(r) > 1.0, ("bf16 gy", r)
    # the last reduction row dropped: n = N - 1 in dgrad, m = M - 1 in wgrad and the bias gradient
    got = (np.matmul(gy[:, :-1], w[:-1]), np.matmul(gy[:-1].T, x[:-1]), gy[:-1].sum(0, dtype=np.float32))
    r = ratios(c, got)
    assert min(r) > 1.0, ("dropped row", r)


def test_zero_products_give_a_zero_bound():
    c = R.case(36, 64, 128, "zero_rows")
    E = c["dgrad"][1]
    assert (E[1::3] == 0).all() and (E[0::3] > 0).all()


GY, W, GX, WS = 0x10004, 0x20000, 0x30000, 0x40000      # gy only 4-byte aligned: legal
EINVAL, EUNSUPPORTED = -1, -4


def dgrad(L, gy=GY, w=W, gx=GX, M=8, N=2, K=8, ws=None, wsb=0):
    return L.m3d_linear_dgrad(C.c_void_p(gy), C.c_void_p(w), C.c_void_p(gx), M, N, K, C.c_void_p(ws), C.c_size_t(wsb), None)


def wgrad(L, gy=GY, x=W, gw=GX, gb=0x50004, M=8, N=2, K=8, ws=None, wsb=0):
    return L.m3d_linear_wgrad(C.c_void_p(gy), C.c_void_p(x), C.c_void_p(gw), C.c_void_p(gb), M, N, K, C.c_void_p(ws), C.c_size_t(wsb), None)


def test_abi_limits_without_a_gpu(L):
    from m3d._lib import SYMBOLS
    for s in ("m3d_linear_dgrad", "m3d_linear_wgrad", "m3d_linear_dgrad_workspace_bytes", "m3d_linear_wgrad_workspace_bytes"):
        assert s in SYMBOLS and hasattr(L, s), s
    split = (260, 128, 4096)                                   # few output tiles: both calls ask for a workspace
    for call, need_of in ((dgrad, L.m3d_linear_dgrad_workspace_bytes), (wgrad, L.m3d_linear_wgrad_workspace_bytes)):
        # M3D_EINVAL
        assert call(L, gy=None) == EINVAL and call(L, **{"w" if call is dgrad else "x": None}) == EINVAL
        assert call(L, **{"gx" if call is dgrad else "gw": None}) == EINVAL
        assert call(L, gy=GY + 2) == EINVAL and call(L, gy=GY + 1) == EINVAL           # not 4-byte aligned
        assert call(L, **{"w" if call is dgrad else "x": W + 2}) == EINVAL
        assert call(L, **{"gx" if call is dgrad else "gw": GX + 3}) == EINVAL
        assert call(L, N=0) == EINVAL and call(L, K=0) == EINVAL and call(L, M=-1) == EINVAL
        need = need_of(*split)
        assert need > 0
        M, N, K = split
        assert call(L, M=M, N=N, K=K, ws=None, wsb=need) == EINVAL                        # no workspace
        assert call(L, M=M, N=N, K=K, ws=WS, wsb=need - 16) == EINVAL                     # smaller than asked for
        assert call(L, M=M, N=N, K=K, ws=WS + 2, wsb=need) == EINVAL
        # M3D_EUNSUPPORTED
        assert call(L, K=6) == EUNSUPPORTED and call(L, K=2) == EUNSUPPORTED
        assert call(L, **{"w" if call is dgrad else "x": W + 4}) == EUNSUPPORTED          # a big operand off a 16-byte boundary
        assert call(L, **{"gx" if call is dgrad else "gw": GX + 8}) == EUNSUPPORTED
        assert call(L, M=M, N=N, K=K, ws=WS + 4, wsb=need) == EUNSUPPORTED
        assert call(L, M=1 << 20, N=1, K=1 << 11) == EUNSUPPORTED                         # x / gx: 2^31 elements
        assert call(L, M=1, N=1 << 20, K=1 << 11) == EUNSUPPORTED                         # W / gw
        assert call(L, M=1 << 16, N=1 << 15, K=4) == EUNSUPPORTED                         # gy
    assert wgrad(L, gb=0x50002) == EINVAL
    # an empty batch: dgrad has nothing to write and looks at no pointer (wgrad zero-fills its outputs: tested on the GPU)
    assert dgrad(L, M=0) == 0 and dgrad(L, gy=None, w=None, gx=None, M=0) == 0


def test_workspace_sizes(L):
    for N, K in ((2, 1024), (12, 1024), (64, 128), (1024, 1024), (256, 2744), (1024, 4096), (4096, 512)):
        for f, cap in ((L.m3d_linear_dgrad_workspace_bytes, lambda M: 64 * M * K * 4),
                       (L.m3d_linear_wgrad_workspace_bytes, lambda M: 64 * (N * K + N) * 4)):
            prev = 0
            for M in range(1, 700):
                b = f(M, N, K)
                assert b % 16 == 0 and b >= prev, (N, K, M, b, prev)
                assert b <= cap(M) + 16                                                   # at most 64 slices
                prev = b
            assert f(0, N, K) == 0
    # a function of the shape only
    assert L.m3d_linear_wgrad_workspace_bytes(128, 1024, 1024) == L.m3d_linear_wgrad_workspace_bytes(128, 1024, 1024)
    # the shipped fc1 shapes have enough tiles: wgrad needs no workspace there
    assert L.m3d_linear_wgrad_workspace_bytes(128, 1024, 87808) == 0 and L.m3d_linear_wgrad_workspace_bytes(256, 1024, 43904) == 0
