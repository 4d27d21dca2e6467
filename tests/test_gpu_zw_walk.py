"""GPU: the persistent unit walk of the f16x2 conv (csrc/conv3d_zw.hip), element by element, over the case table of tests/zw_walk_cases.py
(its properties are proved on the CPU by tests/test_zw_walk_cases_host.py).  The small cases run on the tuning build with the grid
override tune_zw_grid = G, so that a workgroup walks up to all of a launch's ~32 units; the release cases run the stock library's own
walk (3 units per workgroup on 256 CUs).  Every output is allocated here, pre-filled with a NaN sentinel, between guard zones.

 (a) exact on integers under every walk: the result EQUALS the fp64 reference (plain conv; conv + scale + shift + ReLU; max_pool3d of
     that; the transposed conv; the per-window strip conv; strip_prepare: the prepare launch applied to the exact strip) at every G, and
     out_max's largest slot is max |y|;
 (b) walk-independence on fractional data: the bits at every G are the bits at G = units; strip_prepare at G = units is the two
     launches strip + prepare; three runs at G = 1 agree;
 (c) bounded on random data under a walk (G = 1, 3): within zw_contract's E everywhere, exactly the shift (or 0) where C == 0;
 (d) the stock library's own walk on the release cases: exact on integers, bounded, and the tuning build's bits at tune_zw_grid = -1 / 256;
 (e) nn.Conv3d(32, 130) through m3d.compat's training route at 300 units on integers: y and x.grad equal fp64 autograd.

Measured on an MI355X (pytest -s prints them), worst |y^ - y| / E: (c) un-pooled 0.916, dgrad 0.809, pooled 0.772 (all three in the
`quiet` family, where the rounding of the shift add, 2^-24 |y|, is nearly all of the bound; benign and outlier24 stay below 0.1),
strip 0.084; (d) release un-pooled 0.023, pooled 0.022.  The whole file: 125 tests in 4 s."""
import pytest
import torch

import zw_walk_cases as T
from test_gpu_conv_train import SENTINEL, guarded, intact
from test_gpu_f16x2_range import WORST, meets

pytestmark = pytest.mark.gpu

F64 = torch.float64


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as o
    assert torch.cuda.is_available()
    yield o
    for site, r in sorted(WORST.items()):
        if site.startswith("zw walk"):
            print("zw walk: worst |y^ - y| / E  %-28s %.3g" % (site, r))
    _dev.clear()
    torch.cuda.empty_cache()


class grid(object):
    """`with grid(G):` - launches inside run on the tuning build with tune_zw_grid = G; G = None: the release library, no override"""

    def __init__(self, G):
        self.G = G

    def __enter__(self):
        if self.G is not None:
            from m3d import _lib
            self.t = _lib.tuning()
            self.t.__enter__()
            assert _lib.lib().m3d_tuning_build() == 1
            _lib.set_option("tune_zw_grid", self.G)
            assert _lib.get_option("tune_zw_grid") == self.G

    def __exit__(self, *a):
        if self.G is not None:
            torch.cuda.synchronize()
            self.t.__exit__(*a)
        return False


_dev = {}


def device_operands(ops, name, kind, o):
    """the operands of a case on the device, packed once: dict(conv, a, bound, scale, shift[, prep])"""
    key = (name, kind)
    if key not in _dev:
        c = T.CASES[name]
        Z = ops.ZwConv3d
        w = o["w"].cuda()
        d = dict(conv=Z.dgrad_of(w) if c.form == "dgrad" else Z(w), scale=o["scale"].cuda(), shift=o["shift"].cuda())
        if c.form in ("strip", "strip_prepare"):
            P, n = o["a"].shape[0], o["a"].shape[2]
            pitch, lead, L = ops.strip_geometry(n, 2, P)
            assert L == c.shape[5]
            d.update(a=T.strip_of(o["a"], pitch, lead, L).cuda().contiguous(), pitch=pitch, lead=lead, P=P, n=n)
            b = torch.zeros(P, 32)
            b[:, 0] = o["a"].abs().flatten(1).amax(1)
            d["bound"] = b.cuda()
            if c.form == "strip_prepare":
                d["prep"] = {k: v.cuda() for k, v in T.prepare_operands(c).items()}
        else:
            d["a"] = o["a"].cuda()
            d["bound"] = Z.bound_of(d["a"])
            assert float(d["bound"].max()) == float(o["a"].abs().max())
        _dev[key] = d
    return _dev[key]


def launch(ops, name, d, G, epilogue=True):
    """one launch of a case under grid G -> (out, out_max or origin_out or None); the output between guards, the sentinel underneath"""
    c = T.CASES[name]
    B, cin, cout, D, H, W = T.kernel_dims(c)
    pool = c.form == "pool"
    with grid(G):
        if c.form == "strip_prepare":
            p = d["prep"]
            r = d["conv"].strip_prepare(d["a"], (d["P"], cin, d["n"]), p["origin"], p["xnext"], p["scale"], p["norm"], p["up_off"], bounds=d["bound"])
            assert r is not None
            return r
        oshape = (cout, D, H, W) if c.form == "strip" else (B, cout, D // 2, H // 2, W // 2) if pool else (B, cout, D, H, W)
        numel = 1
        for v in oshape:
            numel *= v
        buf, mid = guarded(numel)
        out = mid.view(torch.float32).view(oshape)
        if c.form == "strip":
            got, om = d["conv"].strip(d["a"], d["pitch"], d["P"], out=out, bounds=d["bound"]), None
            assert got is not None
        else:
            kw = dict(scale=d["scale"], shift=d["shift"], relu=(pool or epilogue == "relu")) if epilogue else {}
            got, om = d["conv"](d["a"], d["bound"], pool=pool, out=out, **kw)
        torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    assert intact(buf), (name, G, "a write outside the output")
    never = (mid == SENTINEL).nonzero()
    assert never.numel() == 0, "%s G = %s: %d elements never written, first flat index %d" % (name, G, never.shape[0], int(never[0]))
    return got, om


def windows(d, strip):
    """[P, C, planes, n, n] <- the windows' columns of a strip [C, planes, n, L]"""
    return torch.stack([strip[..., d["lead"] + p * d["pitch"]:d["lead"] + p * d["pitch"] + d["n"]] for p in range(d["P"])])


def same(name, G, got, ref, what, pooled=False, strip=False):
    """bit-equal to the fp64 reference cast to fp32 (test_gpu_direct_conv.same); on a mismatch: how many, where, which channels, and the
    walk unit of the first wrong element (unit u is visited by the workgroup with l0 = u % G, at its iteration u // G)"""
    got, ref = got.cpu(), ref.to(torch.float32)
    assert got.shape == ref.shape, (name, G, what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    c = T.CASES[name]
    bad = (got != ref).nonzero()
    first = bad[0].tolist()
    where = ""
    if not strip:
        idx = first[:2] + [v * (2 if pooled else 1) for v in first[2:]]
        u = T.unit_of(c, idx)
        where = "; unit %d of %d" % (u, c.units) + ("" if G is None else " (walk %d, iteration %d)" % (u % G, u // G))
    raise AssertionError("%s G = %s %s: %d of %d elements differ; first %s got %r want %r; last %s; channels %s%s"
                         % (name, G, what, bad.shape[0], ref.numel(), first, float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
                            bad[-1].tolist(), sorted(set(bad[:, 1].tolist()))[:40], where))


def two_launches(ops, name, d, strip):
    """the prepare launch (m3d_prm_prepare_ex3: pool 0, border 1, quad-aligned strips in and out) on a strip conv's result"""
    c = T.CASES[name]
    p = d["prep"]
    return ops.prm_prepare(strip, p["origin"], False, 1, None, p["xnext"], p["scale"], p["norm"], in_strip=2, out_strip=2,
                           up_off=p["up_off"], dims=(d["P"], T.kernel_dims(c)[2], d["n"]))


SMALL_RUNS = [(n, G) for n, c in T.SMALL.items() for G in T.grids(c)]


# ------------------------------------------------------------------ (a) exact on integers under every walk
@pytest.mark.parametrize("name,G", SMALL_RUNS, ids=["%s-G%d" % r for r in SMALL_RUNS])
def test_exact_on_integers_under_every_walk(ops, name, G):
    c = T.SMALL[name]
    o, plain, full = T.integer_reference(name)
    d = device_operands(ops, name, "int", o)
    if c.form == "strip":
        got, _ = launch(ops, name, d, G)
        same(name, G, windows(d, got), plain, "strip windows", strip=True)
        return
    if c.form == "strip_prepare":
        # the strip conv of this table at G = units is exact (the `strip` case); the fused launch must give what the prepare launch makes
        # of that strip, at every G
        strip, _ = launch(ops, "strip", d, c.units)
        same("strip", c.units, windows(d, strip), plain, "strip windows", strip=True)
        want, want_origin = two_launches(ops, name, d, strip)
        got, origin = launch(ops, name, d, G)
        assert torch.equal(origin, want_origin) and torch.equal(origin.cpu(), d["prep"]["origin"].cpu() - 1)
        same(name, G, got.unsqueeze(0), want.cpu().unsqueeze(0).to(F64), "fused prepare", strip=True)
        assert int((want != 0).sum()) > 0
        return
    pooled = c.form == "pool"
    runs = [("relu", full, "scale, shift, relu" + (", pool" if pooled else ""))]
    if not pooled:
        runs.insert(0, (False, plain, "plain"))
    for epi, ref, what in runs:
        got, om = launch(ops, name, d, G, epilogue=epi)
        same(name, G, got, ref, what, pooled=pooled)
        assert float(om.max()) == float(ref.abs().max()) and bool((om >= 0).all()), (name, G, what, float(om.max()), float(ref.abs().max()))


# ------------------------------------------------------------------ (b) walk-independence, bit for bit
@pytest.mark.parametrize("family", T.WALK_FAMILIES)
@pytest.mark.parametrize("name", list(T.SMALL))
def test_every_walk_gives_the_same_bits(ops, name, family):
    c = T.SMALL[name]
    o = T.random_operands(c, family)
    d = device_operands(ops, name, family, o)
    anchor, extra = launch(ops, name, d, c.units)
    assert bool(torch.isfinite(anchor).all())
    if c.form == "strip_prepare":                        # = the two launches, bit for bit (tests/test_gpu_prm.py has it at the engine level)
        strip, _ = launch(ops, "strip", d, c.units)
        want, want_origin = two_launches(ops, name, d, strip)
        assert torch.equal(extra, want_origin)
        assert torch.equal(anchor, want), (name, family, int((anchor != want).sum()))
        assert int((want != 0).sum()) > 0
    for G in T.grids(c):
        for rep in range(3 if G == 1 else 1):
            got, ex = launch(ops, name, d, G)
            if not torch.equal(got, anchor):
                bad = (got != anchor).nonzero()
                raise AssertionError("%s %s G = %d run %d: %d of %d elements differ from G = units; first %s last %s; channels %s"
                                     % (name, family, G, rep, bad.shape[0], anchor.numel(), bad[0].tolist(), bad[-1].tolist(),
                                        sorted(set(bad[:, anchor.dim() - 4].tolist()))[:40]))
            if c.form == "strip_prepare":
                assert torch.equal(ex, extra)
            elif ex is not None:
                assert torch.equal(ex.max(), extra.max()), (name, family, G)


# ------------------------------------------------------------------ (c) bounded on random data under a walk
def check_contract(ops, name, family, G, site):
    c = T.CASES[name]
    o, res = T.contract(name, family)
    d = device_operands(ops, name, family, o)
    got, _ = launch(ops, name, d, G)
    if c.form == "strip":
        w = windows(d, got)
        for p, (y, E, C) in enumerate(res):
            meets(site, w[p:p + 1], y, E, C)
    else:
        y, E, C = res[0]
        meets(site, got, y, E, C)
    print("%s %s G = %s: worst |y^ - y| / E so far for '%s' %.4f" % (name, family, G, site, WORST[site]))


@pytest.mark.parametrize("G", T.BOUND_GRIDS)
@pytest.mark.parametrize("family", T.BOUND_FAMILIES)
@pytest.mark.parametrize("name", [n for n, c in T.SMALL.items() if c.form != "strip_prepare"])
def test_bounded_on_random_data_under_a_walk(ops, name, family, G):
    check_contract(ops, name, family, G, "zw walk " + T.SMALL[name].form)


# ------------------------------------------------------------------ (d) the stock library's own walk
@pytest.mark.parametrize("name", list(T.RELEASE))
def test_the_stock_librarys_own_walk(ops, name):
    from m3d import _lib
    c = T.RELEASE[name]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    o, plain, full = T.integer_reference(name)
    d = device_operands(ops, name, "int", o)
    units = d["conv"].units(o["a"].shape)
    assert units == c.units
    per = (units + cus - 1) // cus
    assert per >= 2, "%d CUs walk %d units one at a time: this device does not test the walk" % (cus, units)
    assert _lib.lib().m3d_tuning_build() == 0
    pooled = c.form == "pool"
    got, om = launch(ops, name, d, None, epilogue="relu")
    same(name, None, got, full, "scale, shift, relu" + (", pool" if pooled else ""), pooled=pooled)
    assert float(om.max()) == float(full.abs().max())
    check_contract(ops, name, "benign", None, "zw walk release " + c.form)
    o2, _ = T.contract(name, "benign")
    d2 = device_operands(ops, name, "benign", o2)
    stock, som = launch(ops, name, d2, None)
    for G in (-1, 256):
        tuned, tom = launch(ops, name, d2, G)
        assert torch.equal(tuned, stock), (name, G, int((tuned != stock).sum()))
        assert torch.equal(tom.max(), som.max())
    assert _lib.lib().m3d_tuning_build() == 0


# ------------------------------------------------------------------ (e) through the callers
@pytest.fixture
def conv_compat():
    import m3d.compat as c
    c.install_conv3d()
    yield c
    c.set_conv_train("fp32")
    c.set_conv_wgrad("fp32")
    c.uninstall_conv3d()


def test_training_route_exact_on_integers_beyond_one_unit_per_cu(ops, conv_compat):
    """tests/test_gpu_conv_train.py::_step on integers: nn.Conv3d(32, 130) on (2, 9, 17, 50) with set_conv_train("f16x2", min_units = 0):
    300 forward units.  (The backward-data conv of 130 output channels has no f16x2 configuration - 130 % 16 != 0 - and stays on the fp32
    kernel, exact as well; the dgrad pack under a walk is case `dgrad` of the table.)"""
    from m3d import conv_plan as cp
    cin, cout, shape = 32, 130, (2, 9, 17, 50)
    g = torch.Generator().manual_seed(12)
    conv = torch.nn.Conv3d(cin, cout, 3, 1, 1).cuda()
    w = torch.randint(-3, 4, tuple(conv.weight.shape), generator=g).float()
    b = torch.randint(-5, 6, (cout,), generator=g).float()
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    x = torch.randint(0, 8, (shape[0], cin) + shape[1:], generator=g).float()
    r = torch.randint(-7, 8, (shape[0], cout) + shape[1:], generator=g).float()
    assert 3 * 9 * max(cin, cout) * 14 * 9 < 2 ** 24
    conv_compat.set_conv_train("f16x2", min_units=0)
    assert cp.train_conv_kernel("forward", shape[0], cin, cout, *shape[1:], "f16x2", min_units=0) == "f16x2"
    assert ops.ZwConv3d(conv.weight.detach()).units((shape[0], cin) + shape[1:]) == 300
    xr = x.cuda().requires_grad_(True)
    y = conv(xr)
    (y * r.cuda()).sum().backward()
    x64 = x.to(F64).requires_grad_(True)
    y64 = torch.nn.functional.conv3d(x64, w.to(F64), b.to(F64), padding=1)
    (y64 * r.to(F64)).sum().backward()
    assert torch.equal(y.detach().cpu(), y64.detach().float()), int((y.detach().cpu() != y64.detach().float()).sum())
    assert torch.equal(xr.grad.cpu(), x64.grad.float()), int((xr.grad.cpu() != x64.grad.float()).sum())
