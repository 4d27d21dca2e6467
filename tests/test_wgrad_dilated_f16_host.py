"""The dilation-2 narrow-map f16x2 conv weight gradient on the CPU (m3d_conv3d_wgrad_narrow_dilated_f16x2; cases:
tests/wgrad_dilated_f16_cases.py, contract: tests/wgrad_f16x2_contract.py with the dilation-2 op): the exact emulation of the cut meets
the per-element bound with the plan's chain and folds on every case and input family, each mutant of the cut breaks it somewhere, the
library's plan gives the case list the coverage it claims and is the dilation-1 plan, the C entry points refuse what they document
before any pointer is followed (the pointers handed over here lead nowhere), the ops wrappers keep their dilation-1 calls, and
conv_plan.plan_train_conv / the m3d.compat switch route as documented."""
import ctypes as C
import itertools
import random

import pytest
import torch

import wgrad_f16x2_contract as K
import wgrad_dilated_f16_cases as N


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


def plan(L, case, dilation=2):
    v = [C.c_int(0) for _ in range(5)]
    assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(*case, dilation, *[C.byref(a) for a in v]) == 0, case
    return tuple(a.value for a in v)              # tile_z, slots, tiles_per_slot, chain, folds


def plan_d1(L, case):
    v = [C.c_int(0) for _ in range(5)]
    assert L.m3d_conv3d_wgrad_narrow_f16x2_plan(*case, *[C.byref(a) for a in v]) == 0, case
    return tuple(a.value for a in v)


@pytest.fixture(scope="module")
def TZ(L):
    return plan(L, (1, 32, 32, 1, 1, 1))[0]


CASE_NAMES = sorted(N.cases(2))                   # the names do not depend on tile_z


def check(got, y, E):
    return bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


def contract(gy, x, n_acc):
    """K.contract with the dilation-2 op: (fp64 reference, E, C, A, B)"""
    A, B = float(gy.abs().max()), float(x.abs().max())
    y = N.wgrad_op_d2(gy, x)
    Cm, Sa, Sb, n = K.terms(N.wgrad_op_d2, gy, x)
    return y, K.bound(n_acc, Cm, Sa, Sb, n, A, B, y), Cm, A, B


@pytest.mark.parametrize("relu_x", [False, True], ids=["signed_x", "relu_x"])
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_cut_meets_the_bound(L, TZ, name, family, relu_x):
    case = N.cases(TZ)[name]
    _, _, _, chain, folds = plan(L, case)
    gy, x = K.make_inputs(family, case, 5, relu_x)
    y, E, Cm, A, B = contract(gy, x, chain + folds)
    got = K.emulate(N.wgrad_op_d2, gy, x, A, B)
    assert check(got, y, E)
    assert bool((got[Cm == 0] == 0).all())
    for axis, t in N.zero_taps(case):
        assert bool((got.select(axis, t) == 0).all()) and bool((Cm.select(axis, t) == 0).all()), (name, axis, t)
    if family == "zero":
        assert bool((got == 0).all()) and bool((E == 0).all())


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_breaks_the_bound_somewhere(L, TZ, mutant):
    """a bound no mutant violates has no teeth: each mutant of the cut leaves it on at least one of MUTANT_CASES x families"""
    assert K.C1 == 3.01 and N.MUTANT_CASES == ["one_tile", "short", "d1_co64"]
    broke = []
    for name in N.MUTANT_CASES:
        case = N.cases(TZ)[name]
        _, _, _, chain, folds = plan(L, case)
        for family in K.FAMILIES:
            for relu_x in (False, True):
                gy, x = K.make_inputs(family, case, 5, relu_x)
                y, E, _, A, B = contract(gy, x, chain + folds)
                assert check(K.emulate(N.wgrad_op_d2, gy, x, A, B), y, E)              # the true cut holds on these very inputs
                if not check(K.emulate(N.wgrad_op_d2, gy, x, A, B, mutant), y, E):
                    broke.append((name, family, relu_x))
    assert broke, mutant


def test_plan_gives_the_case_list_its_coverage(L, TZ):
    """the coverage rule of the GPU test, proved on the library's own plan: a moved tile size or slot rule fails here"""
    cases = N.cases(TZ)
    assert len(cases) == 12
    P = {n: plan(L, c) for n, c in cases.items()}
    per_tile = TZ * 8 // 2 * 3                                                                # MFMAs per accumulator and tile
    for n, c in cases.items():
        tz, slots, tps, chain, folds = P[n]
        assert tz == TZ and c[5] <= 8, n
        assert (slots, tps) == N.expected_plan(c, TZ), n
        assert chain == tps * per_tile and 0 < chain <= N.CHAIN_LIMIT == 384, n
        assert folds == (slots + 7) // 8 + 7 + 2, n
        assert K.flops(c) <= 1.5e9, n
        assert 64 * c[0] * c[3] * c[4] * c[5] < 2 ** 24, n                                    # integer_inputs qualifies
        assert P[n] == plan(L, c, 1) == plan_d1(L, c), n                                      # the dilation-1 plan, through both entries
        assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(*c, 2) == 1, n
    assert P["one_tile"][1:3] == (1, 1) and N.tiles(cases["one_tile"], TZ) == 1               # exactly one tile: one slot
    assert {P[n][2] for n in cases} >= {1, 2, N.MAX_TILES}                                    # tiles per slot 1, 2 and maximal
    assert P["slot2"][2] == 2 and P["slot2"][1] == 550                                        # many partials per reduce group
    assert P["slot16"][2] == N.MAX_TILES and P["slot16"][3] == N.MAX_TILES * per_tile == 384  # the full chain
    assert 0 < N.tiles(cases["slot16"], TZ) % N.MAX_TILES < N.MAX_TILES and P["slot16"][1] >= 3          # a short last slot
    assert all(cases[n][4] == 1 and cases[n][5] == 1 and cases[n][0] == 1 for n in ("slot2", "slot16"))  # built from D alone
    assert N.tiles(cases["slot2"], TZ) == 1100 and N.tiles(cases["slot16"], TZ) == 8200
    assert {(c[2] // 32, c[1] // 32) for c in cases.values()} >= {(2, 1), (1, 3), (3, 2)}     # 64 <- 32, 32 <- 96, 96 <- 64
    assert cases["roi7_b3"][3:] == (7, 7, 7) and cases["b17"] == (17, 32, 32, 7, 7, 7) and N.tiles(cases["b17"], TZ) % 2 == 0
    # whole zero taps: the axes of extent <= 2
    assert N.zero_taps(cases["one_tile"]) == ([(2, 0), (2, 2)] if TZ <= 2 else [])
    assert N.zero_taps(cases["d1_co64"]) == [(2, 0), (2, 2)] and cases["d1_co64"][3] == 1
    assert N.zero_taps(cases["w2"]) == [(4, 0), (4, 2)] and N.zero_taps(cases["h2"]) == [(3, 0), (3, 2)]
    assert all(N.zero_taps(cases[n]) == [] for n in ("roi7_b3", "full", "short", "ci96", "w3", "b17"))
    # `short`: every extent short, odd H, D = 3 the smallest depth with a product in each z-shifted tap
    B, _, _, D, H, W = cases["short"]
    assert D == 3 and H < 8 and H % 2 == 1 and 2 < W < 8
    assert cases["w3"][5] == 3                                                                # one column pair per x-shifted tap
    # `ci96`: the halo (2 rows, 2 slices = a whole z tile) reaches into neighbours on both sides along y and z
    assert cases["ci96"][1] == 96 and cdiv(cases["ci96"][4], 8) >= 2 and cdiv(cases["ci96"][3], TZ) >= 3
    assert cases["w2"][4] == 9 and cases["w2"][5] == 2 and cases["h2"][4] == 2                # one row in a second y tile
    assert set(N.SENTINEL_CASES) <= set(cases) and N.FAMILY_CASE == "short" and set(N.MUTANT_CASES) <= set(cases)
    assert N.SENTINEL_CASES == ["roi7_b3", "ci96", "w3", "slot2"] and P["slot2"][1] > 1 and P["roi7_b3"][1] > 1


def cdiv(a, b):
    return (a + b - 1) // b


def test_short_and_w3_have_exactly_one_product_plane_in_their_shifted_taps(TZ):
    """the claims of the case table about D = 3 and W = 3, on the reference: a z-shifted tap of `short` pairs one slice with one slice"""
    case = N.cases(TZ)["short"]
    gy, x = K.integer_inputs(case, 2)
    for dz, (zo, zi) in ((0, (2, 0)), (2, (0, 2))):
        gy1, x1 = torch.zeros_like(gy), torch.zeros_like(x)
        gy1[:, :, zo], x1[:, :, zi] = gy[:, :, zo], x[:, :, zi]
        assert torch.equal(N.wgrad_op_d2(gy, x)[:, :, dz], N.wgrad_op_d2(gy1, x1)[:, :, dz])
    case = N.cases(TZ)["w3"]
    gy, x = K.integer_inputs(case, 2)
    for dx, (xo, xi) in ((0, (2, 0)), (2, (0, 2))):
        gy1, x1 = torch.zeros_like(gy), torch.zeros_like(x)
        gy1[..., xo], x1[..., xi] = gy[..., xo], x[..., xi]
        assert torch.equal(N.wgrad_op_d2(gy, x)[..., dx], N.wgrad_op_d2(gy1, x1)[..., dx])


def test_chain_limit_on_the_mask_head_shapes(L, TZ):
    """chain <= 384 on the mask head's per-RoI layers, 7^3 grids; workspace_bytes = slots x 27 cin cout floats"""
    for cin, cout in ((256, 256), (128, 128), (32, 32)):
        for R in (4, 16, 64, 128, 300, 1000):
            s = (R, cin, cout, 7, 7, 7)
            assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(*s, 2) == 1, s
            _, slots, tps, chain, folds = plan(L, s)
            assert 0 < chain <= N.CHAIN_LIMIT and chain == tps * (TZ * 8 // 2 * 3) and slots >= 1, s
            assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*s, 2) == slots * 27 * cin * cout * 4, s
    for n, c in N.cases(TZ).items():
        assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*c, 2) == plan(L, c)[1] * 27 * c[1] * c[2] * 4, n
        assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*c, 1) == L.m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*c), n


def test_supported_agrees_with_the_documented_rule(L, TZ):
    rnd = random.Random(7)
    seen = set()
    for _ in range(4000):
        s = (rnd.choice([0, 1, 2, 5]), rnd.choice([0, 16, 32, 48, 64, 96, 100, 256, 4096, 4128]), rnd.choice([-32, 8, 16, 32, 64, 80, 96, 4096, 4128]),
             rnd.choice([0, 1, 2, 7, 65, 1 << 16]), rnd.choice([-1, 0, 1, 3, 7, 8, 130, 1 << 16]), rnd.choice([0, 1, 3, 7, 8, 9, 16, 1 << 16]))
        dil = rnd.choice([0, 1, 2, 3])
        ok = N.supported_rule(*s, dil, TZ)
        seen.add((dil, s[5], ok))
        assert bool(L.m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(*s, dil)) == ok, (s, dil)
        assert (L.m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*s, dil) > 0) == ok, (s, dil)
        rc = L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(*s, dil, None, None, None, None, None)
        assert rc == (0 if ok else -1 if min(s + (dil,)) < 1 else -4), (s, dil)
    for dil in (1, 2):
        assert (dil, 8, True) in seen and (dil, 9, False) in seen and (dil, 9, True) not in seen
    assert not any(ok for dil, _, ok in seen if dil in (0, 3)) and (0, 8, False) in seen and (3, 8, False) in seen
    sup = lambda *s: bool(L.m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(*s))
    assert sup(1, 32, 32, 7, 7, 8, 2) and not sup(1, 32, 32, 7, 7, 9, 2)
    assert sup(1, 4096, 4096, 7, 7, 7, 2) and not sup(1, 4128, 32, 7, 7, 7, 2) and not sup(1, 32, 4128, 7, 7, 7, 2)
    assert not sup(1, 16, 32, 7, 7, 7, 2) and not sup(1, 32, 16, 7, 7, 7, 2)
    assert not sup(0, 32, 32, 7, 7, 7, 2) and not sup(1, 32, 32, 0, 7, 7, 2) and not sup(1, 32, 32, 7, 0, 7, 2) and not sup(1, 32, 32, 7, 7, 0, 2)
    assert not sup(1, 32, 32, 1 << 20, 1 << 16, 8, 2)                                # 2^32 tiles
    assert not sup(1, 4096, 4096, 1 << 20, 1 << 10, 8, 2)                            # too many workgroups
    assert sup(1000, 256, 256, 7, 7, 7, 2) and sup(1000, 256, 256, 7, 7, 7, 1)
    for dil in (-2, 0, 3, 4, 1 << 20):
        assert not sup(3, 32, 32, 7, 7, 7, dil), dil


def test_every_refusal(L, TZ):
    """M3D_EINVAL -1 / M3D_EUNSUPPORTED -4, each before a pointer is followed or anything is launched"""
    p = lambda a: C.c_void_p(a)
    good = dict(x=p(0x10000), gy=p(0x20000), dw=p(0x30000), xm=p(0x40000), gm=p(0x50000), ws=p(0x60000))
    shape = (1, 32, 32, TZ, 8, 8)
    need = L.m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*shape, 2)
    assert need == 32 * 32 * 27 * 4

    def call(shape=shape, dilation=2, ws_bytes=need, **over):
        a = dict(good, **over)
        return L.m3d_conv3d_wgrad_narrow_dilated_f16x2(a["x"], a["gy"], a["dw"], *shape, dilation, a["xm"], a["gm"], a["ws"],
                                                       C.c_size_t(ws_bytes), None)

    for dil in (1, 2):
        for k in good:
            assert call(dilation=dil, **{k: None}) == -1, k                    # NULL
        for k in ("x", "gy", "dw", "xm", "gm"):
            assert call(dilation=dil, **{k: p(good[k].value + 2)}) == -1, k    # a float pointer off its 4 bytes
        assert call(dilation=dil, ws=p(0x60008)) == -1                         # the workspace off its 16 bytes
        for i in range(6):
            for bad in (0, -3):
                s = list(shape)
                s[i] = bad
                assert call(shape=tuple(s), dilation=dil) == -1, s             # non-positive extents
        assert call(dilation=dil, ws_bytes=need - 1) == -1 and call(dilation=dil, ws_bytes=0) == -1       # a workspace that is too small
        for s in ((1, 32, 32, TZ, 8, 9), (1, 16, 32, TZ, 8, 8), (1, 32, 48, TZ, 8, 8), (1, 4128, 32, TZ, 8, 8), (1, 32, 8192, TZ, 8, 8),
                  (1, 4096, 4096, 1 << 20, 1 << 10, 8)):
            assert call(shape=s, dilation=dil, ws_bytes=1 << 40) == -4, s      # what `supported` rejects
        assert call(shape=(1, 16, 32, TZ, 8, 8), dilation=dil, x=None) == -1   # EINVAL goes first
    for dil in (0, -1, -(1 << 20)):
        assert call(dilation=dil) == -1 and call(dilation=dil, ws_bytes=1 << 40) == -1        # dilation < 1
        assert call(shape=(1, 16, 32, TZ, 8, 8), dilation=dil, ws_bytes=1 << 40) == -1        # EINVAL before EUNSUPPORTED
    for dil in (3, 4, 1 << 20):
        assert call(dilation=dil) == -4 and call(dilation=dil, ws_bytes=1 << 40) == -4        # any other dilation is unsupported
        assert call(dilation=dil, x=None) == -1 and call(dilation=dil, ws=p(0x60008)) == -1   # EINVAL goes first
        assert call(shape=(0, 32, 32, TZ, 8, 8), dilation=dil) == -1
    for s in ((1, 32, 32, TZ, 8, 9), (1, 16, 32, TZ, 8, 8)):
        assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(*s, 2, None, None, None, None, None) == -4
    assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(1, 32, 32, 0, 8, 8, 2, None, None, None, None, None) == -1
    assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(1, 32, 32, TZ, 8, 8, 0, None, None, None, None, None) == -1
    assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(1, 16, 32, TZ, 8, 8, 0, None, None, None, None, None) == -1
    assert L.m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(1, 32, 32, TZ, 8, 8, 3, None, None, None, None, None) == -4


def test_ops_wrappers_and_exports(L, TZ):
    import inspect
    import m3d
    from m3d import ops
    assert m3d.conv3d_wgrad_narrow_f16x2 is ops.conv3d_wgrad_narrow_f16x2
    assert m3d.conv3d_wgrad_narrow_f16x2_supported is ops.conv3d_wgrad_narrow_f16x2_supported
    assert m3d.conv3d_wgrad_narrow_f16x2_plan is ops.conv3d_wgrad_narrow_f16x2_plan
    for fn in (ops.conv3d_wgrad_narrow_f16x2, ops.conv3d_wgrad_narrow_f16x2_supported, ops.conv3d_wgrad_narrow_f16x2_plan):
        assert inspect.signature(fn).parameters["dilation"].default == 1, fn
    assert list(inspect.signature(ops.conv3d_wgrad_narrow_f16x2).parameters) == ["x", "grad_out", "x_max", "gy_max", "dilation"]
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 7, dilation=2) is True
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 7, dilation=1) is True
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 7, dilation=3) is False
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 7, dilation=0) is False
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 9, dilation=2) is False
    got = ops.conv3d_wgrad_narrow_f16x2_plan(3, 32, 32, 7, 7, 7, dilation=2)
    assert got == dict(zip(("tile_z", "slots", "tiles_per_slot", "chain", "folds"), plan(L, (3, 32, 32, 7, 7, 7))))
    assert got == ops.conv3d_wgrad_narrow_f16x2_plan(3, 32, 32, 7, 7, 7)
    for bad in (dict(dilation=3), dict(dilation=0)):
        with pytest.raises(m3d.M3DError):
            ops.conv3d_wgrad_narrow_f16x2_plan(3, 32, 32, 7, 7, 7, **bad)
    with pytest.raises(m3d.M3DError):
        ops.conv3d_wgrad_narrow_f16x2_plan(3, 32, 32, 7, 7, 9, dilation=2)
    import m3d.compat as compat
    for name in ("set_conv_wgrad_dilated_f16", "get_conv_wgrad_dilated_f16"):
        assert callable(getattr(compat, name)), name
    from m3d._lib import SYMBOLS
    for name in ("_supported", "_workspace_bytes", "_plan", ""):
        assert "m3d_conv3d_wgrad_narrow_dilated_f16x2" + name in SYMBOLS and hasattr(L, "m3d_conv3d_wgrad_narrow_dilated_f16x2" + name)


def test_without_the_keyword_the_wrappers_make_the_calls_they_made():
    """on the recording double of the library (tests/conv_record.py): with `dilation` left out, or 1, the three wrappers call the
    dilation-1 entry points and nothing else, with the arguments they always had; with 2 they call the entries that take the dilation"""
    from conv_record import CudaMeta, install
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        from m3d import ops
        names = []
        real = rec.real
        mp.setattr(ops, "lib", lambda: type("Named", (), {"__getattr__": lambda self, n: (names.append(n), getattr(rec, n))[1]})())
        meta = lambda *s: torch.empty(s, device="meta").as_subclass(CudaMeta)
        x, gy, b = meta(3, 32, 7, 7, 7), meta(3, 64, 7, 7, 7), meta(32)
        shape = (3, 32, 64, 7, 7, 7)
        wsb = real.m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*shape)
        OLD = "m3d_conv3d_wgrad_narrow_f16x2"
        NEW = "m3d_conv3d_wgrad_narrow_dilated_f16x2"
        for kw in ({}, dict(dilation=1)):
            names.clear(), rec.take()
            assert ops.conv3d_wgrad_narrow_f16x2_supported(*shape, **kw) is True
            ops.conv3d_wgrad_narrow_f16x2_plan(*shape, **kw)
            dw = ops.conv3d_wgrad_narrow_f16x2(x, gy, b, b, **kw)
            launches, queries = rec.take()
            assert names == [OLD + "_supported", OLD + "_plan", OLD + "_workspace_bytes", OLD] and queries == 3
            assert launches == [[OLD, "ptr", "ptr", "ptr", *shape, "ptr", "ptr", "ptr", wsb, "null"]]
            assert tuple(dw.shape) == (64, 32, 3, 3, 3)
        names.clear(), rec.take()
        assert ops.conv3d_wgrad_narrow_f16x2_supported(*shape, dilation=2) is True
        ops.conv3d_wgrad_narrow_f16x2_plan(*shape, dilation=2)
        ops.conv3d_wgrad_narrow_f16x2(x, gy, b, b, dilation=2)
        launches, queries = rec.take()
        assert names == [NEW + "_supported", NEW + "_plan", NEW + "_workspace_bytes", NEW] and queries == 3
        assert launches == [[NEW, "ptr", "ptr", "ptr", *shape, 2, "ptr", "ptr", "ptr", wsb, "null"]]
        # a missing bound is swept with ZwConv3d.bound_of, at either dilation
        for kw in ({}, dict(dilation=2)):
            rec.take()
            ops.conv3d_wgrad_narrow_f16x2(x, gy, **kw)
            assert [l[0] for l in rec.take()[0]] == ["m3d_conv3d_zw_bound_of", "m3d_conv3d_zw_bound_of", NEW if kw else OLD]


X7, W7 = (4, 32, 7, 7, 7), (64, 32, 3, 3, 3)
NEEDS = (True, True, True)
# (x shape, weight shape): supported at W <= 8 with channels multiples of 32, and not
SHAPES = [((4, 32, 7, 7, 7), (64, 32, 3, 3, 3)), ((300, 256, 7, 7, 7), (256, 256, 3, 3, 3)), ((1, 32, 2, 8, 8), (32, 32, 3, 3, 3)),
          ((4, 32, 7, 7, 9), (64, 32, 3, 3, 3)), ((4, 16, 7, 7, 7), (64, 16, 3, 3, 3)), ((4, 32, 7, 7, 7), (48, 32, 3, 3, 3)),
          ((2, 32, 14, 14, 14), (32, 32, 3, 3, 3))]


def settings(cp):
    for train, narrow, wg, wn, dil in itertools.product(("fp32", "f16x2"), (None, 0), ("fp32", "f16x2"), (False, True), ("torch", "m3d")):
        yield cp.TrainSetting(train=train, min_units=0, narrow=narrow, wgrad=wg, wgrad_narrow=wn, dilated=dil)


def test_the_plan_without_the_keyword_is_todays(L):
    from m3d import conv_plan as cp
    for s in settings(cp):
        for x, w in SHAPES:
            for dilation in (1, 2):
                for needs in (NEEDS, (True, False, True), (False, True, False)):
                    for nf, df in ((None, None), (0, None), (None, 0), (0, 0)):
                        t = s._replace(wgrad_narrow_f16=nf, dilated_f16=df)
                        today = cp.plan_train_conv(t, x, w, dilation, needs)
                        assert cp.plan_train_conv(t._replace(wgrad_dilated_f16=None), x, w, dilation, needs) == today
                        assert today.wgrad != cp.WGRAD_DILATED_F16X2
                        assert cp.plan_train_backward(t._replace(wgrad_dilated_f16=None), x, w, dilation, needs) == tuple(today)[2:]


def test_none_makes_no_further_library_query(L):
    from conv_record import install
    from m3d import conv_plan as cp
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        s = cp.TrainSetting(dilated="m3d")
        for df in (None, 0):
            rec.take()
            cp.plan_train_conv(s._replace(dilated_f16=df), X7, W7, 2, NEEDS)
            q0 = rec.take()[1]
            cp.plan_train_conv(s._replace(dilated_f16=df, wgrad_dilated_f16=None), X7, W7, 2, NEEDS)
            assert rec.take()[1] == q0
            cp.plan_train_conv(s._replace(dilated_f16=df, wgrad_dilated_f16=0), X7, W7, 2, NEEDS)
            assert rec.take()[1] == q0 + 1                                              # the one _supported query
            cp.plan_train_conv(s._replace(dilated_f16=df, wgrad_dilated_f16=0), X7, W7, 2, (True, False, True))
            assert rec.take()[1] == q0                                                  # gw not needed: not asked
        rec.take()
        cp.plan_train_conv(cp.TrainSetting(), X7, W7, 1, NEEDS)
        q1 = rec.take()[1]
        cp.plan_train_conv(cp.TrainSetting()._replace(wgrad_dilated_f16=0), X7, W7, 1, NEEDS)
        assert rec.take()[1] == q1                                                      # dilation 1: not asked either


def test_a_threshold_moves_exactly_the_wgrad_field_of_supported_dilation_2_layers(L, TZ):
    from m3d import conv_plan as cp
    assert cp.WGRAD_DILATED_F16X2 == "f16x2 dilated" and isinstance(cp.WGRAD_DILATED_F16X2_MIN_WORK, int) and cp.WGRAD_DILATED_F16X2_MIN_WORK > 0
    moved = 0
    for s in settings(cp):
        for x, w in SHAPES:
            B, cin, D, H, W = x
            cout = w[0]
            work = B * D * H * W * cin * cout
            takes = bool(L.m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(B, cin, cout, D, H, W, 2))
            assert takes == (W <= 8 and cin % 32 == 0 and cout % 32 == 0), (x, w)
            for nf, df in ((None, None), (0, None), (None, 0), (0, 0)):
                t = s._replace(wgrad_narrow_f16=nf, dilated_f16=df)
                off = cp.plan_train_conv(t, x, w, 2, NEEDS)
                assert off.wgrad == cp.WGRAD_DILATED                                    # wgrad_narrow_f16 keeps not touching dilation 2
                for thr in (0, work):                                                   # at or above the threshold
                    on = cp.plan_train_conv(t._replace(wgrad_dilated_f16=thr), x, w, 2, NEEDS)
                    want = cp.WGRAD_DILATED_F16X2 if takes and s.dilated == "m3d" else cp.WGRAD_DILATED
                    assert on.wgrad == want, (s, x, w, thr)
                    assert on._replace(wgrad=off.wgrad) == off                          # forward, sweep, dgrad, gy_reduce, gb
                    moved += on.wgrad != off.wgrad
                    assert cp.plan_train_backward(t._replace(wgrad_dilated_f16=thr), x, w, 2, NEEDS) == tuple(on)[2:]
                    assert cp.plan_train_backward(s._replace(wgrad_narrow_f16=nf, dilated_f16=df, wgrad_dilated_f16=thr), x, w, 2, NEEDS) == tuple(on)[2:]
                assert cp.plan_train_conv(t._replace(wgrad_dilated_f16=work + 1), x, w, 2, NEEDS) == off        # one product below it
                assert cp.plan_train_conv(t._replace(wgrad_dilated_f16=0), x, w, 2, (True, False, True)).wgrad is None
                # dilation-1 plans ignore the dilated field
                assert cp.plan_train_conv(t._replace(wgrad_dilated_f16=0), x, w, 1, NEEDS) == cp.plan_train_conv(t, x, w, 1, NEEDS)
    assert moved
    d2 = cp.TrainSetting(dilated="m3d")
    assert cp.plan_train_conv(d2._replace(wgrad_narrow_f16=0), X7, W7, 2, NEEDS).wgrad == cp.WGRAD_DILATED
    assert cp.plan_train_conv(d2._replace(wgrad_dilated_f16=0), X7, W7, 2, NEEDS).wgrad == cp.WGRAD_DILATED_F16X2
    assert cp.plan_train_conv(d2._replace(wgrad_narrow_f16=0, wgrad_dilated_f16=0), X7, W7, 1, NEEDS).wgrad == cp.WGRAD_NARROW_F16X2
    # the default threshold: the constant, in products per tap
    w = cp.WGRAD_DILATED_F16X2_MIN_WORK
    R = -(-w // (343 * 256 * 256))
    big = (256, 256, 3, 3, 3)
    assert cp.plan_train_conv(d2._replace(wgrad_dilated_f16=w), (R, 256, 7, 7, 7), big, 2, NEEDS).wgrad == cp.WGRAD_DILATED_F16X2
    if R > 1:
        assert cp.plan_train_conv(d2._replace(wgrad_dilated_f16=w), (R - 1, 256, 7, 7, 7), big, 2, NEEDS).wgrad == cp.WGRAD_DILATED
    # the field lists: the six older switches in their order, then the three thresholds the setting now carries itself
    assert cp.TrainSetting._fields == ("train", "min_units", "narrow", "wgrad", "wgrad_narrow", "dilated",
                                       "wgrad_narrow_f16", "dilated_f16", "wgrad_dilated_f16")
    assert cp.TrainConvPlan._fields == ("forward", "sweep", "dgrad", "wgrad", "gy_reduce", "gb")


def test_the_switch_round_trips_and_install_leaves_it_off(L):
    import m3d.compat as c
    from m3d import conv_plan as cp
    assert c.get_conv_wgrad_dilated_f16() is False and c._setting.wgrad_dilated_f16 is None          # default off
    try:
        assert c.set_conv_wgrad_dilated_f16(True) is False and c.get_conv_wgrad_dilated_f16() is True
        assert c._setting.wgrad_dilated_f16 == cp.WGRAD_DILATED_F16X2_MIN_WORK                       # min_work=None: the constant
        assert c.get_conv_wgrad_narrow_f16() is False and c.get_conv_dilated_f16() is False and c.get_conv_dilated() == "torch"
        c.install_conv3d(), c.install_linear()                  # what install() does to F.conv3d / F.linear leaves it alone
        assert c.get_conv_wgrad_dilated_f16() is True
        assert c.set_conv_wgrad_dilated_f16(True, 0) is True and c._setting.wgrad_dilated_f16 == 0   # 0 routes every supported layer
        assert c.set_conv_wgrad_dilated_f16(True) is True and c._setting.wgrad_dilated_f16 == cp.WGRAD_DILATED_F16X2_MIN_WORK
        assert c.set_conv_wgrad_dilated_f16(False) is True and c.get_conv_wgrad_dilated_f16() is False
        with pytest.raises(ValueError):
            c.set_conv_wgrad_dilated_f16(True, -1)
        assert c.get_conv_wgrad_dilated_f16() is False
        # the neighbours keep their meaning
        assert c.set_conv_wgrad_narrow_f16(True) is False and c.get_conv_wgrad_dilated_f16() is False
        assert c.set_conv_wgrad_narrow_f16(False) is True
        assert c.set_conv_dilated_f16(True) is False and c.get_conv_wgrad_dilated_f16() is False
        assert c.set_conv_dilated_f16(False) is True
        c.uninstall_conv3d(), c.uninstall_linear()
        c.install()
        assert c.get_conv_wgrad_dilated_f16() is False
    finally:
        c.set_conv_wgrad_dilated_f16(False)
        c.set_conv_wgrad_narrow_f16(False)
        c.set_conv_dilated_f16(False)
        c.uninstall_conv3d(), c.uninstall_linear()


def test_the_backward_reads_the_switch_when_it_runs_and_needs_set_conv_dilated():
    """on the recording double: the weight-gradient launch of a dilation-2 layer under set_conv_dilated("m3d") moves with the switch as
    it stands when the backward runs; every other launch stays; without set_conv_dilated("m3d") the switch has no effect"""
    from conv_record import CudaMeta, install
    OLD, NEW, SWEEP = "m3d_conv3d_wgrad_dilated", "m3d_conv3d_wgrad_narrow_dilated_f16x2", "m3d_conv3d_zw_bound_of"
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        from m3d import compat
        mp.setattr(compat, "_orig_conv3d", lambda *a: "torch")
        meta = lambda s, g: torch.empty(s, device="meta").as_subclass(CudaMeta).requires_grad_(g)

        def run(at_forward, at_backward, dilated="m3d", dilated_f16=False, xs=X7, dilation=2):
            compat.set_conv_dilated(dilated), compat.set_conv_dilated_f16(dilated_f16, 0)
            compat.set_conv_wgrad_dilated_f16(*at_forward)
            x, w, b = meta(xs, True), meta((64, 32, 3, 3, 3), True), meta((64,), True)
            rec.take()
            y = compat.conv3d(x, w, b, 1, dilation, dilation, 1)
            fwd = rec.take()[0]
            if isinstance(y, str):
                return "torch", None
            compat.set_conv_wgrad_dilated_f16(*at_backward)
            torch.autograd.grad(y, (x, w, b), torch.empty(y.shape, device="meta").as_subclass(CudaMeta))
            return fwd, rec.take()[0]
        try:
            OFF, ON = (False,), (True, 0)
            f0, b0 = run(OFF, OFF)
            assert [l[0] for l in b0].count(OLD) == 1 and NEW not in [l[0] for l in b0]
            for at_forward in (OFF, ON):
                f1, b1 = run(at_forward, ON)                                            # read when the backward runs
                assert f1 == f0
                names = [l[0] for l in b1]
                i = names.index(NEW)
                assert OLD not in names and names[i - 2:i] == [SWEEP, SWEEP]             # no bound in the step: both operands swept
                assert b1[i][1:] == ["ptr", "ptr", "ptr", 4, 32, 64, 7, 7, 7, 2, "ptr", "ptr", "ptr", b1[i][14], "null"]
                rest = b1[:i - 2] + b1[i + 1:]
                assert rest == [l for l in b0 if l[0] != OLD]                           # every other launch stays
                assert run(at_forward, OFF) == (f0, b0)
            # under set_conv_dilated_f16 the step holds both bounds: no sweep in the backward
            f2, b2 = run(ON, ON, dilated_f16=True)
            names = [l[0] for l in b2]
            assert NEW in names and SWEEP not in names and OLD not in names
            f3, b3 = run(OFF, OFF, dilated_f16=True)
            assert f3 == f2 and [l for l in b2 if l[0] != NEW] == [l for l in b3 if l[0] != OLD]
            # the default threshold keeps this small layer where it was
            assert run((True,), (True,)) == (f0, b0) or 4 * 343 * 32 * 64 >= __import__("m3d").conv_plan.WGRAD_DILATED_F16X2_MIN_WORK
            # without set_conv_dilated("m3d"): torch's own conv, switch on or off
            assert run(ON, ON, dilated="torch") == ("torch", None)
            # a W = 12 dilation-2 layer and a dilation-1 layer are unchanged
            assert run(ON, ON, xs=(2, 32, 4, 6, 12)) == run(OFF, OFF, xs=(2, 32, 4, 6, 12))
            assert run(ON, ON, dilation=1) == run(OFF, OFF, dilation=1)
        finally:
            compat.set_conv_wgrad_dilated_f16(False), compat.set_conv_dilated_f16(False), compat.set_conv_dilated("torch")
