"""GPU: the up-conv's backward on the f16 matrix cores (csrc/upconv3d_bwd_f16.hip) element by element against the f16x2 contract of
tests/upconv_backward_f16_cases.py (n_acc from the library's own _plan), its exactness on integers, its stores, its determinism, its
bounds, what it does with an Inf on either side of the ReLU mask, and its routing through m3d.upconv3d_2x's autograd.

Largest |error| / bound over every case x family, with and without the mask (MI355X): dgrad 0.29 (split, quiet), wgrad 0.84 (one,
quiet: a single product, whose own rounding is most of the bound), gb 0.04."""
import ctypes as C

import numpy as np
import pytest
import torch

import upconv_backward_f16_cases as UC

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC12345                      # a quiet NaN with a payload: "never written"
GUARD = 4096
F64 = torch.float64
SLOTS = 32


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def run(gy, w, x, y=None, gy_max=None, w_max=None, x_max=None):
    from m3d import ops
    gx = ops.upconv3d_2x_dgrad_f16x2(gy, w, y=y, gy_max=gy_max, w_max=w_max)
    gw, gb = ops.upconv3d_2x_wgrad_f16x2(gy, x, y=y, gy_max=gy_max, x_max=x_max)
    return gx, gw, gb


def run_case(c, **kw):
    y = None if c["y"] is None else c["y"].cuda()
    return run(c["gy"].cuda(), c["w"].cuda(), c["x"].cuda(), y=y, **kw)


def plans(shape):
    from m3d import ops
    return {d: ops.upconv3d_2x_backward_f16x2_plan(d, *shape) for d in ("dgrad", "wgrad")}


def check_contract(c, got, what, A=None, B=(None, None)):
    """gx, gW within the f16x2 bound of the library's plan, gb within its fp32 bound; exact zeros where every product is zero"""
    gx, gw, gb = (t.cpu() for t in got)
    R, Cin, Cout, D, H, W = c["shape"]
    assert gx.shape == (R, Cin, D, H, W) and gw.shape == (Cin, Cout, 2, 2, 2) and gb.shape == (Cout,)
    p = plans(c["shape"])
    for (d, t), b in zip((("dgrad", gx), ("wgrad", gw)), B):
        assert p[d]["chain"] <= UC.MAX_CHAIN
        y, E, Cm = UC.contract(c, d, UC.n_acc(p[d]), A=A, B=b)
        r = UC.worst_ratio(t, y, E)
        print("RATIO %s %s: plan %s, largest error / E = %.3f" % (what, d, p[d], r))
        assert bool(torch.isfinite(t).all()), d
        assert bool((t[Cm == 0] == 0).all()), d + ": an output whose products are all zero must be exactly 0"
        assert UC.violations(t, y, E) == 0, (d, r)
    ref, Eb = UC.gb_contract(c, p["wgrad"]["gb_partials"])
    print("RATIO %s gb: largest error / E = %.3f" % (what, UC.worst_ratio(gb, ref, Eb)))
    assert bool((gb[Eb == 0] == 0).all())
    assert UC.violations(gb, ref, Eb) == 0


@pytest.mark.parametrize("masked", (False, True), ids=("plain", "mask"))
@pytest.mark.parametrize("kind", UC.FAMILIES)
@pytest.mark.parametrize("name", list(UC.CASES))
def test_every_element_within_the_contract(name, kind, masked):
    c = UC.case(name, kind, masked)
    got = run_case(c)
    check_contract(c, got, "%s %s %s" % (name, kind, "mask" if masked else "plain"))
    if kind == "dead_channel" and masked:
        assert (bits(got[1])[:, UC.DEAD] == 0).all() and bits(got[2])[UC.DEAD] == 0


@pytest.mark.parametrize("name", list(UC.CASES))
def test_integer_operands_are_bit_exact(name):
    """integers in [-3, 3]: every cut is exact (lo = 0), every product and every partial sum is an integer whose magnitude stays below
    2^24 (at most 9 x 32 928 terms), gb included; with the mask"""
    R, Cin, Cout, D, H, W = UC.CASES[name]
    g = torch.Generator().manual_seed(R + Cin + Cout + W)
    gy, y = (torch.randint(-3, 4, (R, Cout, 2 * D, 2 * H, 2 * W), generator=g).to(torch.float32) for _ in range(2))
    w = torch.randint(-3, 4, (Cin, Cout, 2, 2, 2), generator=g).to(torch.float32)
    x = torch.randint(-3, 4, (R, Cin, D, H, W), generator=g).to(torch.float32)
    gx, gw, gb = run(gy.cuda(), w.cuda(), x.cuda(), y=y.cuda())
    g64 = UC.mask_of(gy, y).to(F64)
    assert float(g64.abs().sum(dim=(0, 2, 3, 4)).max()) < 2 ** 24
    assert torch.equal(gx.cpu().to(F64), UC.dgrad_op(g64, w.to(F64)))
    assert torch.equal(gw.cpu().to(F64), UC.wgrad_op(g64, x.to(F64)))
    assert torch.equal(gb.cpu().to(F64), g64.sum(dim=(0, 2, 3, 4)))


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


@pytest.mark.parametrize("name", ("one", "ragged", "roi_grid", "wide_row", "shipped", "deep", "split"))
def test_stores_stay_inside_outputs_and_workspace(name):
    """NaN-filled guard bands around the three outputs and both workspaces stay as they were; every output element and every element of
    the workspace the call uses (the two swept bounds; the partial sums behind the 256 bytes of bounds) is written; the results are the
    wrapper's bits"""
    from m3d._lib import lib, check
    c = UC.case(name, "benign", True)
    s = R, Cin, Cout, D, H, W = c["shape"]
    L = lib()
    gy, w, x, y = c["gy"].cuda(), c["w"].cuda(), c["x"].cuda(), c["y"].cuda()
    ngx, ngw = R * Cin * D * H * W, Cin * Cout * 8
    bgx, gx = guarded(ngx)
    bgw, gw = guarded(ngw)
    bgb, gb = guarded(Cout)
    p = lambda t: C.c_void_p(t.data_ptr())
    z = C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nd, nw = L.m3d_upconv3d_2x_dgrad_f16x2_workspace_bytes(*s), L.m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(*s)
    assert nd == 256 and nw % 16 == 0 and nw >= 256
    bwd, wsd = guarded(nd // 4)
    bww, wsw = guarded(nw // 4)
    check(L.m3d_upconv3d_2x_dgrad_f16x2(p(gy), p(y), p(w), p(gx), *s, z, z, p(wsd), C.c_size_t(nd), st), "upconv3d_2x_dgrad_f16x2")
    check(L.m3d_upconv3d_2x_wgrad_f16x2(p(gy), p(y), p(x), p(gw), p(gb), *s, z, z, p(wsw), C.c_size_t(nw), st), "upconv3d_2x_wgrad_f16x2")
    torch.cuda.synchronize()
    for buf, n, what in ((bgx, ngx, "gx"), (bgw, ngw, "gw"), (bgb, Cout, "gb")):
        inner = check_guards(buf, n, what)
        assert (inner != NAN_BITS).all(), what + ": an output element was not written"
        assert np.isfinite(inner.view(np.float32)).all(), what + ": a NaN survived"
    slices = plans(s)["wgrad"]["slices"]
    for buf, n, used, what in ((bwd, nd // 4, 0, "dgrad workspace"), (bww, nw // 4, slices * (ngw + Cout) if slices > 1 else 0, "wgrad workspace")):
        inner = check_guards(buf, n, what)
        assert inner[0] != NAN_BITS and inner[SLOTS] != NAN_BITS, what + ": the two swept bounds"
        assert n == 64 + used and (inner[64:] != NAN_BITS).all(), what + ": a partial sum was not written"
        assert np.isfinite(inner[64:].view(np.float32)).all(), what + ": a NaN survived in a partial sum"
    for a, b in zip((gx, gw, gb), run_case(c)):
        assert np.array_equal(bits(a), bits(b).reshape(-1))


@pytest.mark.parametrize("name", ("ragged", "roi_grid", "deep", "split"))
def test_a_loose_bound_meets_its_own_contract(name):
    """bounds given as 4 x the true maxima (two binades of headroom lost): the contract computed with THOSE bounds holds"""
    from m3d import ops
    c = UC.case(name, "benign", True)
    four = lambda t: ops.ZwConv3d.bound_of(t.cuda()) * 4.0
    got = run_case(c, gy_max=four(c["gy"]), w_max=four(c["w"]), x_max=four(c["x"]))
    check_contract(c, got, name + " bounds x 4", A=4 * c["A"], B=(4 * c["B"]["dgrad"], 4 * c["B"]["wgrad"]))


@pytest.mark.parametrize("name", ("ragged", "roi_grid", "shipped"))
def test_given_bounds_equal_swept_bounds(name):
    """gy_max=None (the library's sweep) equals the swept bound passed in - as a slot array with the maximum in any slot, or as one
    float - bit for bit"""
    from m3d import ops
    c = UC.case(name, "benign", True)
    swept = [bits(t) for t in run_case(c)]
    gy, w, x = c["gy"].cuda(), c["w"].cuda(), c["x"].cuda()
    for a, b in zip(swept, run_case(c, gy_max=ops.ZwConv3d.bound_of(gy), w_max=ops.ZwConv3d.bound_of(w), x_max=ops.ZwConv3d.bound_of(x))):
        assert np.array_equal(a, bits(b))

    def slots(t, at):
        out = torch.zeros(SLOTS, device="cuda")
        out[at] = ops.absmax(t)[0]
        out[(at + 5) % SLOTS] = out[at] / 3
        return out
    for a, b in zip(swept, run_case(c, gy_max=slots(gy, 17), w_max=slots(w, SLOTS - 1), x_max=ops.absmax(x))):
        assert np.array_equal(a, bits(b))


@pytest.mark.parametrize("name", list(UC.CASES))
def test_bit_identical_run_to_run(name):
    c = UC.case(name, "heavy", True)
    first = [bits(t) for t in run_case(c)]
    second = [bits(t) for t in run_case(c)]
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    if name in ("roi_grid", "shipped", "split"):
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


@pytest.mark.parametrize("name", ("ragged", "roi_grid"))
def test_an_inf_on_either_side_of_the_mask(name):
    """A masked-out Inf in gy contributes exactly 0: with the bound of the finite values given, the results are the bits of the run
    without it; with the library's own sweep (the bound of the unmasked gy is Inf then) they are finite.  An unmasked Inf makes every
    output it belongs to non-finite: the column of gx, the n of gW, gb[co]."""
    from m3d import ops
    c = UC.case(name, "relu_mask", True)
    gy, y = c["gy"].clone(), c["y"]
    clean = [bits(t) for t in run_case(c, gy_max=ops.ZwConv3d.bound_of(c["gy"].cuda()))]
    dead = torch.nonzero(y.reshape(-1) <= 0)[7].item()
    live = torch.nonzero(y.reshape(-1) > 0)[11].item()
    gy.view(-1)[dead] = float("inf")
    cu = lambda t: t.cuda()
    for a, b in zip(clean, run(cu(gy), cu(c["w"]), cu(c["x"]), y=cu(y), gy_max=ops.ZwConv3d.bound_of(c["gy"].cuda()))):
        assert np.array_equal(a, bits(b))
    for t in run(cu(gy), cu(c["w"]), cu(c["x"]), y=cu(y)):
        assert bool(torch.isfinite(t).all())
    gy.view(-1)[dead] = c["gy"].view(-1)[dead]
    gy.view(-1)[live] = float("inf")
    g64 = UC.mask_of(gy, y).to(F64)
    refs = (UC.dgrad_op(g64, c["w"].to(F64)), UC.wgrad_op(g64, c["x"].to(F64)), g64.sum(dim=(0, 2, 3, 4)))
    for kw in ({}, {"gy_max": ops.ZwConv3d.bound_of(c["gy"].cuda())}):
        for got, ref in zip(run(cu(gy), cu(c["w"]), cu(c["x"]), y=cu(y), **kw), refs):
            bad = ~torch.isfinite(ref)
            assert int(bad.sum()) > 0
            assert bool((~torch.isfinite(got.cpu()[bad])).all())


def test_empty_batch_unsupported_shapes_and_shape_checks():
    from m3d import ops, M3DError
    w = torch.randn(32, 64, 2, 2, 2, device="cuda")
    gy, x = torch.empty(0, 64, 6, 6, 6, device="cuda"), torch.empty(0, 32, 3, 3, 3, device="cuda")
    out = torch.full((32, 64, 2, 2, 2), float("nan"), device="cuda")
    gw, gb = ops.upconv3d_2x_wgrad_f16x2(gy, x, out=out)
    assert gw is out and (bits(gw) == 0).all() and gb.shape == (64,) and (bits(gb) == 0).all()
    assert ops.upconv3d_2x_dgrad_f16x2(gy, w).shape == (0, 32, 3, 3, 3)
    w16 = torch.zeros(16, 32, 2, 2, 2, device="cuda")
    g1 = torch.zeros(1, 32, 2, 2, 2, device="cuda")
    assert not ops.upconv3d_2x_backward_f16x2_supported((1, 16, 1, 1, 1), 32)
    with pytest.raises(M3DError):
        ops.upconv3d_2x_dgrad_f16x2(g1, w16)
    with pytest.raises(M3DError):
        ops.upconv3d_2x_wgrad_f16x2(g1, torch.zeros(1, 16, 1, 1, 1, device="cuda"))
    with pytest.raises(ValueError):
        ops.upconv3d_2x_dgrad_f16x2(torch.zeros(1, 32, 2, 2, 2, device="cuda"), w)              # gy has 32 channels, the weight 64
    with pytest.raises(ValueError):
        ops.upconv3d_2x_wgrad_f16x2(g1, torch.zeros(1, 32, 2, 1, 1, device="cuda"))            # gy is not twice x
    with pytest.raises(ValueError):
        ops.upconv3d_2x_dgrad_f16x2(g1, torch.zeros(32, 32, 2, 2, 2, device="cuda"), y=torch.zeros(1, 32, 2, 2, 4, device="cuda"))
    with pytest.raises(ValueError):
        ops.upconv3d_2x_dgrad_f16x2(g1, torch.zeros(32, 32, 2, 2, 2, device="cuda"), gy_max=torch.zeros(3, device="cuda"))


@pytest.fixture()
def switches():
    import m3d.compat as compat
    prev = compat.set_upconv("m3d"), compat.set_upconv_f16(False)
    yield compat
    compat.set_upconv_backward("fp32")
    compat.set_upconv(prev[0])
    compat.set_upconv_f16(prev[1])
    compat.invalidate_packs()


def _grads(x0, w, b, gy):
    import m3d
    x = x0.detach().clone().requires_grad_(True)
    w.grad = b.grad = None
    y = m3d.upconv3d_2x(x, w, b, relu=True)
    y.backward(gy)
    return y.detach(), (x.grad.detach().clone(), w.grad.detach().clone(), b.grad.detach().clone())


@pytest.mark.parametrize("name", ("roi_grid", "shipped"))
def test_autograd_follows_the_switch(switches, name):
    """Default: gx / gw / gb of m3d.upconv3d_2x are the bits of ops.upconv3d_2x_dgrad / _wgrad.  set_upconv_backward("f16x2",
    min_work=0): the same forward bits, gradients within the contract (the mask is the forward's own output), each f16x2 wrapper called
    once, gy swept once, max|W| from the cache the second time and dropped by invalidate_packs (what Solver.step calls).  With the f16x2
    forward on as well the wgrad takes the bound the forward swept: no sweep of x in the backward."""
    from m3d import ops
    compat = switches
    gy0, w0, x0, _ = UC.make_inputs(name, "benign")
    w = torch.nn.Parameter(w0.cuda())
    b = torch.nn.Parameter(torch.randn(w0.shape[1], generator=torch.Generator().manual_seed(5)).cuda() * 0.1)
    x, gy = x0.cuda(), gy0.cuda()
    assert compat.get_upconv_backward() == "fp32"
    y_off, off = _grads(x, w, b, gy)
    gw_ref, gb_ref = ops.upconv3d_2x_wgrad(gy, x, y=y_off)
    for a, r in zip(off, (ops.upconv3d_2x_dgrad(gy, w.detach(), y=y_off), gw_ref, gb_ref)):
        assert np.array_equal(bits(a), bits(r))

    calls = {"dgrad": 0, "wgrad": 0, "bound_of": 0, "fp32": 0}
    saved = (ops.upconv3d_2x_dgrad_f16x2, ops.upconv3d_2x_wgrad_f16x2, ops.ZwConv3d.bound_of, ops.upconv3d_2x_dgrad, ops.upconv3d_2x_wgrad)

    def counting(key, fn):
        def f(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return f
    ops.upconv3d_2x_dgrad_f16x2, ops.upconv3d_2x_wgrad_f16x2 = counting("dgrad", saved[0]), counting("wgrad", saved[1])
    ops.ZwConv3d.bound_of = staticmethod(counting("bound_of", saved[2]))
    ops.upconv3d_2x_dgrad, ops.upconv3d_2x_wgrad = counting("fp32", saved[3]), counting("fp32", saved[4])
    try:
        compat.invalidate_packs()
        assert compat.set_upconv_backward("f16x2", min_work=0) == "fp32"
        y_on, on = _grads(x, w, b, gy)
        assert np.array_equal(bits(y_on), bits(y_off))                                     # the forward does not change
        assert calls == {"dgrad": 1, "wgrad": 1, "bound_of": 2, "fp32": 0}, calls          # gy once, the weight once
        _, again = _grads(x, w, b, gy)
        assert calls == {"dgrad": 2, "wgrad": 2, "bound_of": 3, "fp32": 0}, calls          # max|W| came from the cache
        for a, r in zip(on, again):
            assert np.array_equal(bits(a), bits(r))
        c = UC.build(UC.CASES[name], gy0, w0, x0, y_on.cpu())
        check_contract(c, on, name + " autograd")
        assert len(compat._upconv_wmax_cache) == 1
        compat.invalidate_packs()
        assert not compat._upconv_wmax_cache
        # the f16x2 forward holds the bound of x: the backward sweeps gy and (after the invalidate) the weight, not x
        compat.set_upconv_f16(True)
        n0 = calls["bound_of"]
        y16, on16 = _grads(x, w, b, gy)
        assert calls["bound_of"] == n0 + 3, calls                                           # x (forward), gy, the weight
        check_contract(UC.build(UC.CASES[name], gy0, w0, x0, y16.cpu()), on16, name + " autograd, f16x2 forward")
        compat.set_upconv_f16(False)
        # back off: the first bits again
        compat.set_upconv_backward("fp32")
        for a, r in zip(off, _grads(x, w, b, gy)[1]):
            assert np.array_equal(bits(a), bits(r))
        assert calls["fp32"] == 2
    finally:
        ops.upconv3d_2x_dgrad_f16x2, ops.upconv3d_2x_wgrad_f16x2, _, ops.upconv3d_2x_dgrad, ops.upconv3d_2x_wgrad = saved
        del ops.ZwConv3d.bound_of                                                           # the shadow: the base class's staticmethod is back
