"""GPU: the linear backward on the f16 matrix cores (csrc/fc_backward_f16.hip) element by element against the f16x2 contract of
tests/linear_backward_f16_cases.py (n_acc from the library's own _plan), its exactness on integers and zeros, its stores, its
determinism, its bounds, what it does with a NaN, and its routing through m3d.compat."""
import ctypes as C

import numpy as np
import pytest
import torch

import linear_backward_f16_cases as LC
import linear_backward_reference as R

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC12345                      # a quiet NaN with a payload: "never written"
GUARD = 4096
F64 = torch.float64


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def run(gy, w, x, gy_max=None, w_max=None, x_max=None):
    from m3d import ops
    gx = ops.linear_dgrad_f16x2(gy, w, gy_max, w_max)
    gw, gb = ops.linear_wgrad_f16x2(gy, x, gy_max, x_max)
    return gx, gw, gb


def run_case(c, **kw):
    return run(c["gy"].cuda(), c["w"].cuda(), c["x"].cuda(), **kw)


def plans(M, N, K):
    from m3d import ops
    return {"dgrad": ops.linear_dgrad_f16x2_plan(M, N, K), "wgrad": ops.linear_wgrad_f16x2_plan(M, N, K)}


@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("M,N,K", LC.CASES)
def test_every_element_within_the_contract(M, N, K, kind):
    c = LC.case(M, N, K, kind)
    gx, gw, gb = run_case(c)
    assert gx.shape == (M, K) and gw.shape == (N, K) and gb.shape == (N,)
    p = plans(M, N, K)
    for name, got in (("dgrad", gx.cpu()), ("wgrad", gw.cpu())):
        assert p[name]["chain"] <= LC.MAX_CHAIN
        y, E, Cm = LC.contract(c, name, LC.n_acc(p[name]))
        r = LC.worst_ratio(got, y, E)
        print("(%d,%d,%d) %s %s: plan %s, largest error / E = %.3f" % (M, N, K, kind, name, p[name], r))
        assert bool(torch.isfinite(got).all()), name
        assert bool((got[Cm == 0] == 0).all()), name + ": an output whose products are all zero must be exactly 0"
        assert LC.violations(got, y, E) == 0, (name, r)
    ref, Eb = c["bias"]
    got = gb.cpu().numpy()
    print("(%d,%d,%d) %s bias: largest error / E = %.3f" % (M, N, K, kind, R.worst_ratio(got, ref, Eb)))
    assert (got[Eb == 0] == 0).all()
    assert (np.abs(got.astype(np.float64) - ref) <= Eb).all()


@pytest.mark.parametrize("M,N,K", LC.CASES)
def test_integer_operands_are_bit_exact(M, N, K):
    """integers in [-8, 8]: every cut is exact (lo = 0), every product and every partial sum is an integer below 2^24 x the scales"""
    g = torch.Generator().manual_seed(M + N + K)
    gy, w, x = (torch.randint(-8, 9, s, generator=g).to(torch.float32) for s in ((M, N), (N, K), (M, K)))
    gx, gw, gb = run(gy.cuda(), w.cuda(), x.cuda())
    assert torch.equal(gx.cpu().to(F64), gy.to(F64) @ w.to(F64))
    assert torch.equal(gw.cpu().to(F64), gy.to(F64).T @ x.to(F64))
    assert torch.equal(gb.cpu().to(F64), gy.to(F64).sum(0))


def test_all_zero_products_are_exactly_zero():
    """zero rows of gy (dgrad rows, no wgrad term), zero columns of gy (wgrad rows, gb), zero columns of W and x: exact zeros, +0 bits"""
    M, N, K = 77, 96, 160
    c = LC.case(M, N, K, "benign")
    gy, w, x = c["gy"].clone(), c["w"].clone(), c["x"].clone()
    gy[5] = 0.0
    gy[:, 7] = 0.0
    w[:, 33] = 0.0
    x[:, 129] = 0.0
    gx, gw, gb = run(gy.cuda(), w.cuda(), x.cuda())
    assert (bits(gx)[5] == 0).all() and (bits(gx)[:, 33] == 0).all()
    assert (bits(gw)[7] == 0).all() and (bits(gw)[:, 129] == 0).all() and bits(gb)[7] == 0
    z = torch.zeros
    for t in run(z(M, N).cuda(), w.cuda(), x.cuda()) + run(gy.cuda(), z(N, K).cuda(), z(M, K).cuda())[:2]:
        assert (bits(t) == 0).all()


def guarded(n):
    """(whole buffer as int32, the n-float output inside it): NaN bit pattern everywhere, GUARD floats on both sides, 16-byte aligned"""
    buf = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device="cuda")
    out = buf[GUARD:GUARD + n].view(torch.float32)
    assert out.data_ptr() % 16 == 0
    return buf, out


def check_guards(buf, n, what):
    b = buf.cpu().numpy()
    assert (b[:GUARD] == NAN_BITS).all() and (b[GUARD + n:] == NAN_BITS).all(), what + ": a guard was written"
    return b[GUARD:GUARD + n]


@pytest.mark.parametrize("M,N,K", [(77, 96, 160), (129, 192, 2752), (33, 1024, 1024), (260, 128, 4096), (40, 2112, 64)])
def test_stores_stay_inside_outputs_and_workspace(M, N, K):
    """NaN-filled guard bands around the three outputs and both workspaces stay as they were; every output element and every element of
    the used workspace (the partial sums behind the 256 bytes of bounds) is written"""
    from m3d._lib import lib, check
    c = LC.case(M, N, K, "benign")
    L = lib()
    gy, w, x = c["gy"].cuda(), c["w"].cuda(), c["x"].cuda()
    bgx, gx = guarded(M * K)
    bgw, gw = guarded(N * K)
    bgb, gb = guarded(N)
    p = lambda t: C.c_void_p(t.data_ptr())
    z = C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nd, nw = L.m3d_linear_dgrad_f16x2_workspace_bytes(M, N, K), L.m3d_linear_wgrad_f16x2_workspace_bytes(M, N, K)
    assert nd % 16 == 0 and nw % 16 == 0 and nd >= 256 and nw >= 256
    bwd, wsd = guarded(nd // 4)
    bww, wsw = guarded(nw // 4)
    check(L.m3d_linear_dgrad_f16x2(p(gy), p(w), p(gx), M, N, K, z, 0, z, 0, p(wsd), C.c_size_t(nd), st), "linear_dgrad_f16x2")
    check(L.m3d_linear_wgrad_f16x2(p(gy), p(x), p(gw), p(gb), M, N, K, z, 0, z, 0, p(wsw), C.c_size_t(nw), st), "linear_wgrad_f16x2")
    torch.cuda.synchronize()
    for buf, n, what in ((bgx, M * K, "gx"), (bgw, N * K, "gw"), (bgb, N, "gb")):
        assert (check_guards(buf, n, what) != NAN_BITS).all(), what + ": an output element was not written"
    pl = plans(M, N, K)
    for buf, n, used, what in ((bwd, nd // 4, pl["dgrad"]["slices"] * M * K, "dgrad workspace"),
                               (bww, nw // 4, pl["wgrad"]["slices"] * (N * K + N), "wgrad workspace")):
        inner = check_guards(buf, n, what)
        assert (inner[:2] != NAN_BITS).all(), what + ": the two swept bounds"
        if n > 64:                                                # a split reduction: partial sums behind the bounds
            assert n == 64 + used and (inner[64:] != NAN_BITS).all(), what + ": a partial sum was not written"
    ref = run_case(c)
    for a, b in zip((gx.view(M, K), gw.view(N, K), gb), ref):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("M,N,K", LC.CASES)
def test_bit_identical_run_to_run(M, N, K):
    c = LC.case(M, N, K, "heavy")
    first = [bits(t) for t in run_case(c)]
    second = [bits(t) for t in run_case(c)]
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    if (M, N, K) in ((33, 1024, 1024), (260, 128, 4096)):
        # another stream, after an unrelated allocation has moved the allocator on
        keep = torch.empty(3 * 1000 * 1000 + 17, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            third = run_case(c)
        s.synchronize()
        for a, b in zip(first, [bits(t) for t in third]):
            assert np.array_equal(a, b)
        del keep


@pytest.mark.parametrize("M,N,K", [(77, 96, 160), (33, 1024, 1024)])
def test_given_bounds_equal_swept_bounds(M, N, K):
    """a bound equal to the swept one - as one float, or as the largest of a slot array - gives the same bits; so does any bound with
    the same power of two"""
    from m3d import ops
    c = LC.case(M, N, K, "benign")
    gy, w, x = c["gy"].cuda(), c["w"].cuda(), c["x"].cuda()
    swept = [bits(t) for t in run(gy, w, x)]
    one = dict(gy_max=ops.absmax(gy), w_max=ops.absmax(w), x_max=ops.absmax(x))
    for a, b in zip(swept, run(gy, w, x, **one)):
        assert np.array_equal(a, bits(b))

    def slots(v, at):
        t = torch.zeros(ops.ZwConv3d.SLOTS, device="cuda")
        t[at] = v
        t[(at + 5) % ops.ZwConv3d.SLOTS] = v / 3
        return t
    many = dict(gy_max=slots(one["gy_max"][0], 0), w_max=slots(one["w_max"][0], 17), x_max=slots(one["x_max"][0], ops.ZwConv3d.SLOTS - 1))
    for a, b in zip(swept, run(gy, w, x, **many)):
        assert np.array_equal(a, bits(b))


@pytest.mark.parametrize("M,N,K", [(77, 96, 160), (33, 1024, 1024), (40, 2112, 64)])
def test_a_nan_reaches_every_output_it_belongs_to(M, N, K):
    """One NaN in gy and one in W / x: every output whose fp64 reference is non-finite is non-finite (nothing is lost in the sweep or the
    cut).  Those are: row m of gx and row n of gw and gb[n] for gy[m, n] = NaN; column k of gx for W[., k] = NaN; column k of gw for
    x[., k] = NaN - a NaN times a zero is a NaN in the reference and on the matrix cores alike.  (The bound is a NaN then, the scale
    2^-114: outputs without a NaN term are not held to the contract.)"""
    c = LC.case(M, N, K, "zero_rows")
    gy, w, x = c["gy"].clone(), c["w"].clone(), c["x"].clone()
    gy[M // 2, N - 3] = float("nan")
    w[N // 3, K - 1] = float("nan")
    x[0, 2] = float("nan")
    gx, gw, gb = (t.cpu() for t in run(gy.cuda(), w.cuda(), x.cuda()))
    for got, ref in ((gx, gy.to(F64) @ w.to(F64)), (gw, gy.to(F64).T @ x.to(F64)), (gb, gy.to(F64).sum(0))):
        bad = ~torch.isfinite(ref)
        assert int(bad.sum()) > 0
        assert bool((~torch.isfinite(got[bad])).all())
    assert int((~torch.isfinite(gy.to(F64) @ w.to(F64))).sum()) == K + M - 1
    # the same with the bounds given (finite, from the clean tensors): the cut alone carries the NaN
    from m3d import ops
    clean = dict(gy_max=ops.absmax(c["gy"].cuda()), w_max=ops.absmax(c["w"].cuda()), x_max=ops.absmax(c["x"].cuda()))
    gx2, gw2, gb2 = (t.cpu() for t in run(gy.cuda(), w.cuda(), x.cuda(), **clean))
    for got, ref in ((gx2, gy.to(F64) @ w.to(F64)), (gw2, gy.to(F64).T @ x.to(F64)), (gb2, gy.to(F64).sum(0))):
        assert bool((~torch.isfinite(got[~torch.isfinite(ref)])).all())


def test_empty_batch():
    from m3d import ops
    N, K = 64, 1024
    gy, x, w = torch.empty(0, N, device="cuda"), torch.empty(0, K, device="cuda"), torch.randn(N, K, device="cuda")
    out = torch.full((N, K), float("nan"), device="cuda")
    gw, gb = ops.linear_wgrad_f16x2(gy, x, out=out)
    assert gw is out and (bits(gw) == 0).all() and gb.shape == (N,) and (bits(gb) == 0).all()
    assert ops.linear_dgrad_f16x2(gy, w).shape == (0, K)


def test_unsupported_shape_is_an_error():
    from m3d import ops, M3DError
    gy, w = torch.zeros(4, 12, device="cuda"), torch.zeros(12, 64, device="cuda")
    assert not ops.linear_backward_f16x2_supported(4, 12, 64) and ops.linear_dgrad_f16x2_plan(4, 12, 64) is None
    with pytest.raises(M3DError):
        ops.linear_dgrad_f16x2(gy, w)
    with pytest.raises(M3DError):
        ops.linear_wgrad_f16x2(gy, torch.zeros(4, 64, device="cuda"))


@pytest.fixture()
def linear_installed():
    import m3d.compat as compat
    was = compat._orig_linear is not None
    compat.install_linear()
    yield compat
    compat.set_linear_backward("fp32")
    if not was:
        compat.uninstall_linear()


def _layer_backward(lin, x0, gy):
    x = x0.detach().clone().requires_grad_(True)
    for p in lin.parameters():
        p.grad = None
    lin(x).backward(gy)
    return x.grad.detach().clone(), lin.weight.grad.detach().clone(), lin.bias.grad.detach().clone()


def test_compat_switch(linear_installed):
    """Off: the backward of an nn.Linear is the fp32 kernels' bits.  On (min_work = 0): gx / gw within the contract, gb within its bound,
    the two f16x2 wrappers called once each, gy swept once, the cached max|W| refreshed after an in-place weight update; a layer the
    library refuses (N = 12) stays on the fp32 kernels."""
    import torch.nn as nn
    from m3d import ops
    compat = linear_installed
    M, N, K = 77, 96, 160
    c = LC.case(M, N, K, "benign")
    lin = nn.Linear(K, N).cuda()
    with torch.no_grad():
        lin.weight.copy_(c["w"].cuda())
    x0, gy = c["x"].cuda(), c["gy"].cuda()
    assert compat.get_linear_backward() == "fp32"
    off = _layer_backward(lin, x0, gy)
    gw_ref, gb_ref = ops.linear_wgrad(gy, x0)
    for a, b in zip(off, (ops.linear_dgrad(gy, lin.weight.detach()), gw_ref, gb_ref)):
        assert np.array_equal(bits(a), bits(b))

    calls = {"dgrad": 0, "wgrad": 0, "absmax": 0, "fp32": 0}
    saved = (ops.linear_dgrad_f16x2, ops.linear_wgrad_f16x2, ops.absmax, ops.linear_dgrad, ops.linear_wgrad)

    def counting(name, fn):
        def f(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return f
    ops.linear_dgrad_f16x2, ops.linear_wgrad_f16x2, ops.absmax = counting("dgrad", saved[0]), counting("wgrad", saved[1]), counting("absmax", saved[2])
    ops.linear_dgrad, ops.linear_wgrad = counting("fp32", saved[3]), counting("fp32", saved[4])
    try:
        compat.invalidate_packs()
        assert compat.set_linear_backward("f16x2", min_work=0) == "fp32"
        on = _layer_backward(lin, x0, gy)
        assert calls == {"dgrad": 1, "wgrad": 1, "absmax": 2, "fp32": 0}, calls           # gy once, the weight once
        again = _layer_backward(lin, x0, gy)
        assert calls == {"dgrad": 2, "wgrad": 2, "absmax": 3, "fp32": 0}, calls           # max|W| came from the cache
        for a, b in zip(on, again):
            assert np.array_equal(bits(a), bits(b))
        p = plans(M, N, K)
        for name, got in (("dgrad", on[0].cpu()), ("wgrad", on[1].cpu())):
            y, E, _ = LC.contract(c, name, LC.n_acc(p[name]))
            assert LC.violations(got, y, E) == 0, name
        ref, Eb = c["bias"]
        assert (np.abs(on[2].cpu().numpy().astype(np.float64) - ref) <= Eb).all()
        # an in-place update through the parameter bumps its version: a weight 2^12 times larger must not meet the old bound
        with torch.no_grad():
            lin.weight.mul_(4096.0)
        big = _layer_backward(lin, x0, gy)
        assert calls["absmax"] == 5, calls
        assert bool(torch.isfinite(big[0]).all())
        assert np.array_equal(bits(big[0]), bits(on[0] * 4096.0))                        # a power of two: the same cut, the same sum
        assert len(compat._wmax_cache) == 1
        compat.invalidate_packs()
        assert not compat._wmax_cache
        # a head the library refuses stays where it was
        head = nn.Linear(K, 12).cuda()
        n0 = calls["fp32"]
        _layer_backward(head, x0, torch.randn(M, 12, device="cuda"))
        assert calls["fp32"] == n0 + 2 and calls["dgrad"] == 3
        # back off: the first bits again
        compat.set_linear_backward("fp32")
        with torch.no_grad():
            lin.weight.copy_(c["w"].cuda())
        for a, b in zip(off, _layer_backward(lin, x0, gy)):
            assert np.array_equal(bits(a), bits(b))
    finally:
        ops.linear_dgrad_f16x2, ops.linear_wgrad_f16x2, ops.absmax, ops.linear_dgrad, ops.linear_wgrad = saved
