"""GPU: the box head's linear backward (csrc/fc_backward.hip) element by element against the derived fp64 bound of
tests/linear_backward_reference.py, its determinism, its stores, its routing through m3d.compat and its memory.

The cases (M, N, K) are the smallest at which each mechanism can go wrong: (1,2,8) one row, one quad; (36,64,128) one tile; (77,2,1024),
(77,12,1024) the heads - odd M, gy rows that are not 16-byte multiples; (128,256,2744) K = 8 x 343, a multiple of 4 but not of 32;
(129,130,2744) ragged in all three dimensions, two tiles each way; (33,1024,1024) fc2 - few output tiles, so the reduction is split;
(260,128,4096) M > 128 - row tiles share a W panel and the wgrad reduction is longer than two chunks."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_backward_reference as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC12345                      # a quiet NaN with a payload: "never written"
GUARD = 4096


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                   # a copy: the shared reference arrays are read-only


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def run(c):
    from m3d import ops
    gy, w, x = dev(c["gy"]), dev(c["w"]), dev(c["x"])
    gx = ops.linear_dgrad(gy, w)
    gw, gb = ops.linear_wgrad(gy, x)
    return gx, gw, gb


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("M,N,K", R.CASES)
def test_every_element_within_the_bound(M, N, K, kind):
    c = R.case(M, N, K, kind)
    gx, gw, gb = run(c)
    assert gx.shape == (M, K) and gw.shape == (N, K) and gb.shape == (N,)
    got = {"dgrad": gx.cpu().numpy(), "wgrad": gw.cpu().numpy(), "bias": gb.cpu().numpy()}
    r = {k: R.worst_ratio(got[k], *c[k]) for k in got}
    print("(%d,%d,%d) %s: largest error / E  dgrad %.3f  wgrad %.3f  bias %.3f" % (M, N, K, kind, r["dgrad"], r["wgrad"], r["bias"]))
    for k in got:
        ref, E = c[k]
        assert np.isfinite(got[k]).all(), k
        assert (got[k][E == 0] == 0).all(), k + ": an output whose products are all zero must be exactly 0"
        assert (np.abs(got[k].astype(np.float64) - ref) <= E).all(), (k, r[k])


@pytest.mark.parametrize("M,N,K", R.CASES)
def test_bit_identical_run_to_run(M, N, K):
    c = R.case(M, N, K, "randn")
    first = [bits(t) for t in run(c)]
    second = [bits(t) for t in run(c)]
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    if (M, N, K) == (33, 1024, 1024):
        # another stream, after an unrelated allocation has moved the allocator on
        keep = torch.empty(3 * 1000 * 1000 + 17, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            third = run(c)
        s.synchronize()
        for a, b in zip(first, [bits(t) for t in third]):
            assert np.array_equal(a, b)
        del keep


def guarded(n):
    """(whole buffer as int32, the n-float output inside it): NaN bit pattern everywhere, GUARD floats on both sides, 16-byte aligned"""
    buf = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + n].view(torch.float32)
    assert out.data_ptr() % 16 == 0
    return buf, out


def check_guarded(buf, n, what):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == NAN_BITS).all() and (b[GUARD + n:] == NAN_BITS).all(), what + ": a guard was written"
    assert (b[GUARD:GUARD + n] != NAN_BITS).all(), what + ": an output element was not written"


@pytest.mark.parametrize("M,N,K", [(129, 130, 2744), (77, 2, 1024)])
def test_stores_stay_inside_the_outputs(M, N, K):
    from m3d._lib import lib, check
    c = R.case(M, N, K, "randn")
    L = lib()
    holder = torch.zeros(M * N + 8, device="cuda")
    off = 1 + (-(holder.data_ptr() // 4) % 4)                     # 4 bytes past a 16-byte boundary
    gy = holder[off:off + M * N].view(M, N)
    gy.copy_(dev(c["gy"]))
    assert gy.data_ptr() % 16 == 4
    w, x = dev(c["w"]), dev(c["x"])
    bgx, gx = guarded(M * K)
    bgw, gw = guarded(N * K)
    bgb, gb = guarded(N)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nd, nw = L.m3d_linear_dgrad_workspace_bytes(M, N, K), L.m3d_linear_wgrad_workspace_bytes(M, N, K)
    bwd, wsd = guarded(max(nd, 16) // 4)
    bww, wsw = guarded(max(nw, 16) // 4)
    check(L.m3d_linear_dgrad(p(gy), p(w), p(gx), M, N, K, p(wsd), C.c_size_t(nd), st), "linear_dgrad")
    check(L.m3d_linear_wgrad(p(gy), p(x), p(gw), p(gb), M, N, K, p(wsw), C.c_size_t(nw), st), "linear_wgrad")
    torch.cuda.synchronize()
    check_guarded(bgx, M * K, "gx")
    check_guarded(bgw, N * K, "gw")
    check_guarded(bgb, N, "gb")
    for buf, n, what in ((bwd, max(nd, 16) // 4, "dgrad workspace"), (bww, max(nw, 16) // 4, "wgrad workspace")):
        b = buf.cpu().numpy()
        assert (b[:GUARD] == NAN_BITS).all() and (b[GUARD + n:] == NAN_BITS).all(), what + ": a guard was written"
    for got, k in ((gx.view(M, K), "dgrad"), (gw.view(N, K), "wgrad"), (gb, "bias")):
        ref, E = c[k]
        assert (np.abs(got.cpu().numpy().astype(np.float64) - ref) <= E).all(), k


@pytest.fixture()
def linear_installed():
    import m3d.compat as compat
    was = compat._orig_linear is not None
    compat.install_linear()
    yield compat
    if not was:
        compat.uninstall_linear()


def test_backward_routes_to_the_two_kernels(linear_installed):
    import torch.nn as nn
    from m3d import ops
    compat = linear_installed
    torch.manual_seed(3)
    for K, N, M in ((1024, 2, 77), (2744, 64, 36)):
        lin = nn.Linear(K, N).cuda()
        x = torch.randn(M, K, device="cuda", requires_grad=True)
        y = lin(x)
        gy = torch.randn_like(y)
        calls = {"dgrad": 0, "wgrad": 0, "linear": 0, "matmul": 0}
        saved = (ops.linear_dgrad, ops.linear_wgrad, ops.linear, torch.matmul, torch.Tensor.__matmul__)

        def counting(name, fn):
            def f(*a, **k):
                calls[name] += 1
                return fn(*a, **k)
            return f
        ops.linear_dgrad, ops.linear_wgrad, ops.linear = counting("dgrad", saved[0]), counting("wgrad", saved[1]), counting("linear", saved[2])
        torch.matmul, torch.Tensor.__matmul__ = counting("matmul", saved[3]), counting("matmul", saved[4])
        try:
            y.backward(gy)
        finally:
            ops.linear_dgrad, ops.linear_wgrad, ops.linear, torch.matmul, torch.Tensor.__matmul__ = saved
        assert calls == {"dgrad": 1, "wgrad": 1, "linear": 0, "matmul": 0}, calls
        compat.uninstall_linear()
        try:
            xr = x.detach().clone().requires_grad_(True)
            lr = nn.Linear(K, N).cuda()
            lr.load_state_dict(lin.state_dict())
            lr(xr).backward(gy)
        finally:
            compat.install_linear()
        for a, b in ((x.grad, xr.grad), (lin.weight.grad, lr.weight.grad), (lin.bias.grad, lr.bias.grad)):
            assert torch.allclose(a.detach(), b.detach(), rtol=1e-4, atol=1e-5 * float(b.detach().abs().max()))


def test_backward_makes_no_weight_sized_temporary(linear_installed):
    """Linear(2744, 1024), 128 rows: the weight is 11.2 MB.  The peak over backward() stays below the three gradients, the (larger of
    the two) workspaces and 2 MB; a transposed copy of the weight would add 11.2 MB."""
    import torch.nn as nn
    from m3d._lib import lib
    M, K, N = 128, 2744, 1024
    torch.manual_seed(4)
    lin = nn.Linear(K, N).cuda()
    x = torch.randn(M, K, device="cuda", requires_grad=True)
    y = lin(x)
    gy = torch.randn_like(y)
    ws = max(lib().m3d_linear_dgrad_workspace_bytes(M, N, K), lib().m3d_linear_wgrad_workspace_bytes(M, N, K))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    y.backward(gy)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    allowed = 4 * (M * K + N * K + N) + ws + (2 << 20)
    print("backward peak %.1f MB, allowed %.1f MB (workspace %.1f MB)" % (peak / 1e6, allowed / 1e6, ws / 1e6))
    assert x.grad is not None and lin.weight.grad is not None and lin.bias.grad is not None
    assert peak < allowed


def test_empty_batch():
    from m3d import ops
    N, K = 12, 1024
    gy, x, w = torch.empty(0, N, device="cuda"), torch.empty(0, K, device="cuda"), torch.randn(N, K, device="cuda")
    out = torch.full((N, K), float("nan"), device="cuda")
    gw, gb = ops.linear_wgrad(gy, x, out=out)
    assert gw is out and (bits(gw) == 0).all() and gb.shape == (N,) and (bits(gb) == 0).all()
    gw2, gb2 = ops.linear_wgrad(gy, x, bias=False)
    assert gb2 is None and (bits(gw2) == 0).all()
    assert ops.linear_dgrad(gy, w).shape == (0, K)
