"""CPU: the accuracy contract of the up-conv's f16x2 backward (tests/upconv_backward_f16_cases.py) - its fp64 references equal torch's
fp64 autograd, the exact-sum emulation of the cut is inside the bound, every mutant leaves it; the library's host functions
(_supported, _plan, workspace sizes, refusals) equal their documented rules and the cases reach the mechanisms they are named for; the
planner routes only what it should.  No GPU is touched: the entry points refuse before any pointer is followed."""
import ctypes as C
import itertools

import pytest
import torch

import upconv_backward_f16_cases as UC

EINVAL, EUNSUPPORTED = -1, -4
F64 = torch.float64


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


def lib_plans(L, shape):
    """[(rc, plan)] of dgrad and wgrad from the library's host-only calls"""
    out = []
    for fn, keys in ((L.m3d_upconv3d_2x_dgrad_f16x2_plan, ("slices", "chain", "folds")),
                     (L.m3d_upconv3d_2x_wgrad_f16x2_plan, ("slices", "chain", "folds", "gb_partials"))):
        v = [C.c_int(-7) for _ in keys]
        rc = fn(*shape, *[C.byref(a) for a in v])
        out.append((rc, dict(zip(keys, (a.value for a in v)))))
    return out


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize("masked", (False, True))
@pytest.mark.parametrize("name", list(UC.CASES))
def test_references_equal_torch_autograd(name, masked):
    """gx, gW, gb of the case module against the fp64 autograd of conv_transpose3d (+ relu: with a bias that puts the forward's output
    above 0 exactly where the case's mask y is)"""
    c = UC.case(name, "relu_mask", masked)
    x = c["x"].to(F64).requires_grad_(True)
    w = c["w"].to(F64).requires_grad_(True)
    b = torch.zeros(w.shape[1], dtype=F64, requires_grad=True)
    out = torch.nn.functional.conv_transpose3d(x, w, b, stride=2)
    if masked:
        # relu's gradient is a select on the sign of its input: shift the input so that its sign is the sign of the case's y
        out = torch.relu(out - out.detach() + c["y"].to(F64))
    out.backward(c["gy"].to(F64))
    for got, ref in ((c["dgrad"][0], x.grad), (c["wgrad"][0], w.grad), (c["gb"][0], b.grad)):
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0)


# ------------------------------------------------------------------ the contract against the emulation
@pytest.mark.parametrize("kind", UC.FAMILIES)
@pytest.mark.parametrize("name", list(UC.CASES))
def test_emulation_meets_the_contract(name, kind):
    """the exact sum of the three products is inside the bound for ANY plan: n_acc = 0; with the mask where the family has one"""
    c = UC.case(name, kind, kind in ("relu_mask", "dead_channel"))
    for d in ("dgrad", "wgrad"):
        y, E, Cm = UC.contract(c, d, 0)
        got = UC.emulate(c, d)
        r = UC.worst_ratio(got, y, E)
        print("%s %s %s: emulation, largest error / E = %.3f" % (name, kind, d, r))
        assert UC.violations(got, y, E) == 0, (d, r)
        assert bool((got[Cm == 0] == 0).all()), d
    if kind == "dead_channel":
        assert bool((c["wgrad"][0][:, UC.DEAD] == 0).all()) and float(c["gb"][0][UC.DEAD]) == 0.0
        assert bool((c["wgrad"][1][:, UC.DEAD] == 0).all())           # C == 0: the bound there is 0


# (mutant, case, family) at which the mutant must leave the bound the kernel is held to at that case (n_acc of the library's own plan)
MUTANT_SITES = [("hi_only", "ragged", "benign"), ("hi_only", "roi_grid", "heavy"), ("drop_hilo", "ragged", "benign"),
                ("drop_hilo", "roi_grid", "relu_mask"), ("lo_unscaled", "ragged", "benign"), ("lo_unscaled", "roi_grid", "heavy"),
                ("swap_bc", "ragged", "benign"), ("swap_bc", "one", "heavy"), ("no_mask", "ragged", "relu_mask"),
                ("no_mask", "roi_grid", "dead_channel")]


@pytest.mark.parametrize("mutant,name,kind", MUTANT_SITES)
def test_mutants_violate_the_contract(L, mutant, name, kind):
    c = UC.case(name, kind, True)
    (_, pd), (_, pw) = lib_plans(L, UC.CASES[name])
    for d, p in (("dgrad", pd), ("wgrad", pw)):
        y, E, _ = UC.contract(c, d, UC.n_acc(p))
        assert UC.violations(UC.emulate(c, d, mutant), y, E) > 0, (mutant, d)


def test_every_mutant_is_named():
    assert {m for m, _, _ in MUTANT_SITES} == set(UC.MUTANTS) | {"swap_bc", "no_mask"}


# ------------------------------------------------------------------ the host functions against a restatement of their rules
def supported_rule(R, Cin, Cout, D, H, W):
    if min(R, Cin, Cout, D, H, W) < 1 or Cin % 32 or Cout % 32:
        return False
    V = D * H * W
    return R * Cin * V < 2 ** 31 and R * Cout * 8 * V < 2 ** 31 and Cin * Cout * 8 < 2 ** 31


def chain_rule(chunks, slices):
    """6 MFMAs per 32-deep chunk, a fold every 64 chunks"""
    cps = -(-chunks // slices)
    return dict(slices=slices, chain=6 * min(cps, 64), folds=-(-cps // 64) if cps > 64 else 0)


def dgrad_rule(R, Cin, Cout, D, H, W):
    """upconv3d_bwd_f16.hip dgrad_plan: chunks of 4 output channels, never split"""
    return chain_rule(Cout // 4, 1)


def wgrad_rule(R, Cin, Cout, D, H, W):
    """upconv3d_bwd_f16.hip wgrad_plan: 128 x 128 tiles, chunks of 32 columns, 512 workgroup slots, at most 16 slices of about four
    chunks or more; gb: 4 k-groups x 8 parities, then the slices"""
    tiles, chunks = -(-Cin // 128) * (8 * Cout // 128), -(-(R * D * H * W) // 32)
    s = 1 if tiles >= 512 else 512 // tiles
    s = max(min(s, 16, chunks // 4 + 1), 1)
    return dict(chain_rule(chunks, s), gb_partials=32 + s)


SWEEP = list(itertools.product((1, 2, 16, 64, 300), (16, 32, 48, 64, 256, 288), (8, 32, 33, 256, 512), ((1, 1, 1), (2, 3, 5), (7, 7, 7), (14, 14, 14))))


def test_supported_and_plan_equal_their_rules(L):
    shapes = list(UC.CASES.values()) + [(R, ci, co) + v for R, ci, co, v in SWEEP] + [(2 ** 20, 32, 32, 7, 7, 7), (1, 32, 2 ** 23, 1, 1, 1),
                                                                                    (0, 32, 32, 7, 7, 7), (1, 32, 32, 0, 7, 7), (1, 32, 32, 7, 7, 0)]
    for s in shapes:
        want = supported_rule(*s)
        assert bool(L.m3d_upconv3d_2x_backward_f16x2_supported(*s)) == want, s
        (rd, pd), (rw, pw) = lib_plans(L, s)
        nd, nw = L.m3d_upconv3d_2x_dgrad_f16x2_workspace_bytes(*s), L.m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(*s)
        if not want:
            assert rd == rw == (EINVAL if min(s) < 1 else EUNSUPPORTED), s
            assert nd == 0 and nw == 0
            continue
        assert rd == rw == 0
        assert pd == dgrad_rule(*s), (s, pd)
        assert pw == wgrad_rule(*s), (s, pw)
        for p in (pd, pw):
            assert 1 <= p["slices"] <= 16 and 6 <= p["chain"] <= UC.MAX_CHAIN and p["folds"] >= 0
        R, Cin, Cout = s[:3]
        assert nd == 256
        assert nw == 256 + (pw["slices"] * (Cin * 8 * Cout + Cout) * 4 if pw["slices"] > 1 else 0) and nw % 16 == 0
    assert L.m3d_upconv3d_2x_dgrad_f16x2_plan(1, 32, 32, 7, 7, 7, None, None, None) == 0          # any output pointer may be NULL
    assert L.m3d_upconv3d_2x_wgrad_f16x2_plan(1, 32, 32, 7, 7, 7, None, None, None, None) == 0


def test_supported_edges(L):
    """the rule's edges: Cin = 16 and Cout = 16 (the forward's kernel takes Cin = 16, this one does not), zero extents, R = 0"""
    ok = L.m3d_upconv3d_2x_backward_f16x2_supported
    assert ok(1, 32, 32, 1, 1, 1) and ok(300, 256, 256, 7, 7, 7)
    assert not ok(1, 16, 32, 7, 7, 7) and not ok(1, 32, 16, 7, 7, 7) and not ok(1, 48, 32, 7, 7, 7) and not ok(1, 32, 40, 7, 7, 7)
    assert not ok(0, 32, 32, 7, 7, 7) and not ok(1, 32, 32, 0, 7, 7) and not ok(1, 32, 32, 7, 0, 7) and not ok(1, 32, 32, 7, 7, 0)
    assert not ok(-1, 32, 32, 7, 7, 7) and not ok(1, 0, 32, 7, 7, 7)


def test_the_cases_reach_what_they_are_for(L):
    """the fold, the split and the walk the case table names are what the plans and the tiling say"""
    plan = lambda name: [p for _, p in lib_plans(L, UC.CASES[name])]
    d, w = plan("deep")
    assert 3 * 8 * UC.CASES["deep"][2] // 16 > UC.MAX_CHAIN and d["chain"] == UC.MAX_CHAIN and d["folds"] >= 1
    d, w = plan("split")
    assert w["slices"] >= 2 and w["folds"] >= 1 and w["chain"] == UC.MAX_CHAIN
    R, _, _, D, H, W = UC.CASES["walk"]
    cols = R * D * H * W
    assert -(-cols // 64) > 512 and cols % 64 != 0                     # dgrad: more 64-column tiles than resident slots, the last ragged
    assert plan("walk")[1]["slices"] >= 2
    R, _, _, D, H, W = UC.CASES["one"]
    assert R * D * H * W == 1                                          # a single column against the 16-deep step
    R, _, _, D, H, W = UC.CASES["ragged"]
    assert (D * H * W) % 64 != 0 and R * D * H * W > 64                # a column tile spans RoIs
    assert UC.CASES["wide_row"][5] > 32 and (7 * 7 * 7 * 4) % 16 != 0
    assert plan("shipped")[0] == dict(slices=1, chain=384, folds=0)   # the shipped dgrad: exactly one full chain, no fold


def test_refusals_follow_no_pointer(L):
    """every pointer NULL (and, where one is needed to get past the NULL check, a pointer nothing may follow): the refusal is the return code"""
    z, bad = C.c_void_p(0), C.c_void_p(16)
    sz = C.c_size_t(1 << 30)
    dg = lambda s, p=z, ws=sz: L.m3d_upconv3d_2x_dgrad_f16x2(p, z, p, p, *s, z, z, p, ws, z)
    wg = lambda s, p=z, ws=sz: L.m3d_upconv3d_2x_wgrad_f16x2(p, z, p, p, z, *s, z, z, p, ws, z)
    good = (4, 32, 64, 2, 3, 5)
    for f in (dg, wg):
        for s in ((-1, 32, 32, 7, 7, 7), (4, 0, 32, 7, 7, 7), (4, 32, 0, 7, 7, 7), (4, 32, 32, 0, 7, 7), (4, 32, 32, 7, 7, 0)):
            assert f(s) == EINVAL, s
        for s in ((4, 16, 32, 7, 7, 7), (4, 32, 16, 7, 7, 7), (4, 33, 32, 7, 7, 7), (2 ** 20, 32, 32, 7, 7, 7)):
            assert f(s) == EUNSUPPORTED, s
            assert f(s, bad) == EUNSUPPORTED, s
        assert f(good) == EINVAL                                                   # supported shape, NULL operands
        assert f(good, bad, C.c_size_t(255)) == EINVAL                             # a workspace that is too small
        assert f(good, C.c_void_p(18)) == EINVAL                                   # not 4-byte aligned
        assert f(good, C.c_void_p(20)) == EUNSUPPORTED                             # not 16-byte aligned
    assert dg((0, 32, 32, 7, 7, 7)) == 0                                           # as m3d_upconv3d_2x_dgrad: nothing to do
    assert wg((0, 32, 32, 7, 7, 7)) == EINVAL                                      # as m3d_upconv3d_2x_wgrad: d_gw is needed to zero it
    assert wg((0, 16, 32, 7, 7, 7)) == EUNSUPPORTED
    need = L.m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(*UC.CASES["roi_grid"])
    assert need > 256 and wg(UC.CASES["roi_grid"], bad, C.c_size_t(need - 1)) == EINVAL


# ------------------------------------------------------------------ the planner and the switch
def test_planner_routes_only_supported_shapes_at_or_above_the_thresholds(L):
    from m3d import conv_plan as cp
    mins = {"dgrad": cp.UPCONV_BWD_F16_MIN_DGRAD, "wgrad": cp.UPCONV_BWD_F16_MIN_WGRAD}
    assert cp.UPCONV_BWD_F16_MIN == mins
    for s in list(UC.CASES.values()) + [(R, ci, co) + v for R, ci, co, v in SWEEP] + [(4, 256, 256, 7, 7, 7), (64, 256, 256, 7, 7, 7)]:
        R, Cin, Cout, D, H, W = s
        work = R * D * H * W * Cin * 8 * Cout
        ok = supported_rule(*s)
        for d in ("dgrad", "wgrad"):
            assert cp.upconv_backward_kernel(d, *s, ("fp32", None)) == "fp32"
            assert cp.upconv_backward_kernel(d, *s, ("fp32", 0)) == "fp32"                 # the setting is off: every shape stays
            assert cp.upconv_backward_kernel(d, *s, ("f16x2", 0)) == ("f16x2" if ok else "fp32"), s
            want = "f16x2" if ok and mins[d] is not None and work >= mins[d] else "fp32"
            assert cp.upconv_backward_kernel(d, *s, ("f16x2", None)) == want, (d, s)       # below the threshold: fp32
            assert cp.upconv_backward_kernel(d, *s, ("f16x2", work + 1)) == "fp32"
    for d in ("dgrad", "wgrad"):
        if mins[d] is not None:
            assert mins[d] > 0
            assert cp.upconv_backward_kernel(d, 1, 32, 32, 1, 1, 1, ("f16x2", None)) == "fp32"
    with pytest.raises(ValueError):
        cp.upconv_backward_kernel("forward", 1, 32, 32, 1, 1, 1, ("f16x2", 0))
    with pytest.raises(ValueError):
        cp.upconv_backward_kernel("dgrad", 1, 32, 32, 1, 1, 1, ("bf16", 0))


def test_switch_defaults_to_fp32_and_install_leaves_it():
    import m3d.compat as compat
    assert compat.get_upconv_backward() == "fp32" and compat._upconv_backward == ("fp32", None)
    prev = compat.set_upconv_backward("f16x2", min_work=0)
    try:
        assert prev == "fp32" and compat.get_upconv_backward() == "f16x2" and compat._upconv_backward == ("f16x2", 0)
        with pytest.raises(ValueError):
            compat.set_upconv_backward("f16")
        with pytest.raises(ValueError):
            compat.set_upconv_backward("f16x2", min_work=-1)
    finally:
        compat.set_upconv_backward("fp32")
    assert compat.get_upconv_backward() == "fp32"


def test_python_wrappers_check_shapes():
    """shape checks raise ValueError before anything needs a GPU tensor's contents (the fp32 wrappers' rule); plan names its directions"""
    from m3d import ops
    assert ops.upconv3d_2x_backward_f16x2_supported((1, 32, 7, 7, 7), 32) and not ops.upconv3d_2x_backward_f16x2_supported((1, 16, 7, 7, 7), 32)
    assert not ops.upconv3d_2x_backward_f16x2_supported((1, 32, 7, 7), 32)
    assert ops.upconv3d_2x_backward_f16x2_plan("dgrad", 1, 16, 32, 7, 7, 7) is None
    assert set(ops.upconv3d_2x_backward_f16x2_plan("wgrad", 2, 32, 32, 7, 7, 7)) == {"slices", "chain", "folds", "gb_partials"}
    with pytest.raises(ValueError):
        ops.upconv3d_2x_backward_f16x2_plan("forward", 1, 32, 32, 7, 7, 7)
    import m3d
    for n in ("upconv3d_2x_dgrad_f16x2", "upconv3d_2x_wgrad_f16x2", "upconv3d_2x_backward_f16x2_supported", "upconv3d_2x_backward_f16x2_plan"):
        assert getattr(m3d, n) is getattr(ops, n)
