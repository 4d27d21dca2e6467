"""The narrow-map f16x2 conv weight gradient on the CPU (m3d_conv3d_wgrad_narrow_f16x2; cases: tests/wgrad_narrow_f16_cases.py, contract:
tests/wgrad_f16x2_contract.py): the exact emulation of the cut meets the per-element bound with the new plan's chain and folds on every
case and input family, each mutant of the cut breaks it somewhere, the library's plan gives the case list the coverage it claims, the C
entry points refuse what they document before any pointer is followed (the pointers handed over here lead nowhere), and
conv_plan.wgrad_kernel / the m3d.compat switch route as documented."""
import ctypes as C
import random

import pytest
import torch

import wgrad_f16x2_contract as K
import wgrad_narrow_f16_cases as N


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


def plan(L, case):
    v = [C.c_int(0) for _ in range(5)]
    assert L.m3d_conv3d_wgrad_narrow_f16x2_plan(*case, *[C.byref(a) for a in v]) == 0, case
    return tuple(a.value for a in v)              # tile_z, slots, tiles_per_slot, chain, folds


@pytest.fixture(scope="module")
def TZ(L):
    return plan(L, (1, 32, 32, 1, 1, 1))[0]


CASE_NAMES = sorted(N.cases(2))                   # the names do not depend on tile_z


def check(got, y, E):
    return bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


@pytest.mark.parametrize("relu_x", [False, True], ids=["signed_x", "relu_x"])
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_cut_meets_the_bound(L, TZ, name, family, relu_x):
    case = N.cases(TZ)[name]
    _, _, _, chain, folds = plan(L, case)
    gy, x = K.make_inputs(family, case, 5, relu_x)
    y, E, Cm, A, B = K.contract(gy, x, chain + folds)
    got = K.emulate(K.wgrad_op, gy, x, A, B)
    assert check(got, y, E)
    assert bool((got[Cm == 0] == 0).all())
    if family == "zero":
        assert bool((got == 0).all()) and bool((E == 0).all())


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_breaks_the_bound_somewhere(L, TZ, mutant):
    """a bound no mutant violates has no teeth: each mutant of the cut leaves it on at least one of MUTANT_CASES x families"""
    assert K.C1 == 3.01 and len(N.MUTANT_CASES) == 3
    broke = []
    for name in N.MUTANT_CASES:
        case = N.cases(TZ)[name]
        _, _, _, chain, folds = plan(L, case)
        for family in K.FAMILIES:
            for relu_x in (False, True):
                gy, x = K.make_inputs(family, case, 5, relu_x)
                y, E, _, A, B = K.contract(gy, x, chain + folds)
                assert check(K.emulate(K.wgrad_op, gy, x, A, B), y, E)              # the true cut holds on these very inputs
                if not check(K.emulate(K.wgrad_op, gy, x, A, B, mutant), y, E):
                    broke.append((name, family, relu_x))
    assert broke, mutant


def test_plan_gives_the_case_list_its_coverage(L, TZ):
    """the coverage rule of the GPU test, proved on the library's own plan: a moved tile size or slot rule fails here"""
    cases = N.cases(TZ)
    P = {n: plan(L, c) for n, c in cases.items()}
    per_tile = TZ * 8 // 2 * 3                                                                # MFMAs per accumulator and tile
    for n, c in cases.items():
        tz, slots, tps, chain, folds = P[n]
        assert tz == TZ and c[5] <= 8, n
        assert (slots, tps) == N.expected_plan(c, TZ), n
        assert chain == tps * per_tile and 0 < chain <= N.CHAIN_LIMIT, n
        assert folds == (slots + 7) // 8 + 7 + 2, n
        assert K.flops(c) <= 1.5e9, n
        assert 64 * c[0] * c[3] * c[4] * c[5] < 2 ** 24, n                                    # integer_inputs qualifies
    assert P["one_tile"][1:3] == (1, 1) and N.tiles(cases["one_tile"], TZ) == 1               # exactly one tile: one slot
    assert {P[n][2] for n in cases} >= {1, 2, N.MAX_TILES}                                    # tiles per slot 1, 2 and maximal
    assert P["slot2"][2] == 2 and P["slot2"][1] >= 8 * 8                                      # many partials per reduce group
    assert P["slot16"][2] == N.MAX_TILES and P["slot16"][3] == N.MAX_TILES * per_tile         # the full chain
    assert 0 < N.tiles(cases["slot16"], TZ) % N.MAX_TILES < N.MAX_TILES and P["slot16"][1] >= 3          # a short last slot
    assert all(cases[n][4] == 1 and cases[n][5] == 1 and cases[n][0] == 1 for n in ("slot2", "slot16"))  # built from D alone
    assert 1000 <= N.tiles(cases["slot2"], TZ) <= 1200 and 8000 <= N.tiles(cases["slot16"], TZ) <= 8400
    assert max(c[1] // 32 for c in cases.values()) >= 2 and max(c[2] // 32 for c in cases.values()) >= 2
    assert {(c[2] // 32, c[1] // 32) for c in cases.values()} >= {(2, 1), (1, 3), (3, 2)}     # 64 <- 32, 32 <- 96, 96 <- 64
    assert cases["roi7_b3"][3:] == (7, 7, 7) and cases["b17"][0] == 17
    assert cases["d1_co64"][3] == 1 and cases["w1"][5] == 1 and cases["w3"][5] == 3
    B, _, _, D, H, W = cases["short"]
    assert D < 8 and H < 8 and H % 2 == 1 and W < 8                                           # the last k-step's second row is outside
    assert N.tiles(cases["ci96"], TZ) >= 4 and cases["ci96"][4] > 8                           # several y and z tiles
    assert set(N.SENTINEL_CASES) <= set(cases) and N.FAMILY_CASE in cases and set(N.MUTANT_CASES) <= set(cases)
    assert P["slot2"][1] > 1 and cases["ci96"][1] == 96                                       # sentinels: multi-slot, three cin blocks


def test_chain_limit_on_the_per_roi_shapes(L, TZ):
    """chain <= 384 on the per-RoI layers of the conv box head and of the mask head, 7^3 grids"""
    for cin, cout in ((256, 128), (128, 128), (256, 256)):
        for R in (16, 64, 128, 300, 1000):
            s = (R, cin, cout, 7, 7, 7)
            assert L.m3d_conv3d_wgrad_narrow_f16x2_supported(*s) == 1, s
            _, slots, tps, chain, folds = plan(L, s)
            assert 0 < chain <= N.CHAIN_LIMIT and chain == tps * (TZ * 8 // 2 * 3) and slots >= 1, s
            assert L.m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*s) == slots * 27 * cin * cout * 4, s
    for n, c in N.cases(TZ).items():
        assert 0 < plan(L, c)[3] <= N.CHAIN_LIMIT, n


def test_workspace_is_slots_times_the_gradient(L, TZ):
    for n, c in N.cases(TZ).items():
        assert L.m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*c) == plan(L, c)[1] * 27 * c[1] * c[2] * 4, n


def test_supported_agrees_with_the_documented_rule(L, TZ):
    rnd = random.Random(7)
    seen = set()
    for _ in range(3000):
        s = (rnd.choice([0, 1, 2, 5]), rnd.choice([0, 16, 32, 48, 64, 96, 100, 256, 4096, 4128]), rnd.choice([-32, 8, 16, 32, 64, 80, 96, 4096, 4128]),
             rnd.choice([0, 1, 2, 7, 65, 1 << 16]), rnd.choice([-1, 0, 1, 3, 7, 8, 130, 1 << 16]), rnd.choice([0, 1, 3, 7, 8, 9, 16, 1 << 16]))
        ok = N.supported_rule(*s, TZ)
        seen.add((s[5], ok))
        assert bool(L.m3d_conv3d_wgrad_narrow_f16x2_supported(*s)) == ok, s
        assert (L.m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*s) > 0) == ok, s
        rc = L.m3d_conv3d_wgrad_narrow_f16x2_plan(*s, None, None, None, None, None)
        assert rc == (0 if ok else -1 if min(s) < 1 else -4), s
    assert (8, True) in seen and (9, False) in seen and (9, True) not in seen
    sup = lambda *s: bool(L.m3d_conv3d_wgrad_narrow_f16x2_supported(*s))
    assert sup(1, 32, 32, 7, 7, 8) and not sup(1, 32, 32, 7, 7, 9)
    assert sup(1, 4096, 4096, 7, 7, 7) and not sup(1, 4128, 32, 7, 7, 7) and not sup(1, 32, 4128, 7, 7, 7)
    assert not sup(1, 16, 32, 7, 7, 7) and not sup(1, 32, 16, 7, 7, 7)
    assert not sup(0, 32, 32, 7, 7, 7) and not sup(1, 32, 32, 0, 7, 7) and not sup(1, 32, 32, 7, 0, 7) and not sup(1, 32, 32, 7, 7, 0)
    assert not sup(1, 32, 32, 1 << 20, 1 << 16, 8)                                   # 2^32 tiles
    assert not sup(1, 4096, 4096, 1 << 20, 1 << 10, 8)                               # too many workgroups
    assert sup(1000, 256, 256, 7, 7, 7)


def test_every_refusal(L, TZ):
    """M3D_EINVAL -1 / M3D_EUNSUPPORTED -4, each before a pointer is followed or anything is launched"""
    p = lambda a: C.c_void_p(a)
    good = dict(x=p(0x10000), gy=p(0x20000), dw=p(0x30000), xm=p(0x40000), gm=p(0x50000), ws=p(0x60000))
    shape = (1, 32, 32, TZ, 8, 8)
    need = L.m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*shape)
    assert need == 32 * 32 * 27 * 4

    def call(shape=shape, ws_bytes=need, **over):
        a = dict(good, **over)
        return L.m3d_conv3d_wgrad_narrow_f16x2(a["x"], a["gy"], a["dw"], *shape, a["xm"], a["gm"], a["ws"], C.c_size_t(ws_bytes), None)

    for k in good:
        assert call(**{k: None}) == -1, k                                  # NULL
    for k in ("x", "gy", "dw", "xm", "gm"):
        assert call(**{k: p(good[k].value + 2)}) == -1, k                  # a float pointer off its 4 bytes
    assert call(ws=p(0x60008)) == -1                                       # the workspace off its 16 bytes
    for i in range(6):
        for bad in (0, -3):
            s = list(shape)
            s[i] = bad
            assert call(shape=tuple(s)) == -1, s                           # non-positive extents
    assert call(ws_bytes=need - 1) == -1 and call(ws_bytes=0) == -1        # a workspace that is too small
    for s in ((1, 32, 32, TZ, 8, 9), (1, 16, 32, TZ, 8, 8), (1, 32, 48, TZ, 8, 8), (1, 4128, 32, TZ, 8, 8), (1, 32, 8192, TZ, 8, 8),
              (1, 4096, 4096, 1 << 20, 1 << 10, 8)):
        assert call(shape=s, ws_bytes=1 << 40) == -4, s                    # what `supported` rejects
    assert call(shape=(1, 16, 32, TZ, 8, 8), x=None) == -1                 # EINVAL goes first
    for s in ((1, 32, 32, TZ, 8, 9), (1, 16, 32, TZ, 8, 8)):
        assert L.m3d_conv3d_wgrad_narrow_f16x2_plan(*s, None, None, None, None, None) == -4
    assert L.m3d_conv3d_wgrad_narrow_f16x2_plan(1, 32, 32, 0, 8, 8, None, None, None, None, None) == -1


def test_ops_wrappers_and_exports(L, TZ):
    import m3d
    from m3d import ops
    assert m3d.conv3d_wgrad_narrow_f16x2 is ops.conv3d_wgrad_narrow_f16x2
    assert m3d.conv3d_wgrad_narrow_f16x2_supported is ops.conv3d_wgrad_narrow_f16x2_supported
    assert m3d.conv3d_wgrad_narrow_f16x2_plan is ops.conv3d_wgrad_narrow_f16x2_plan
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 7) is True
    assert ops.conv3d_wgrad_narrow_f16x2_supported(3, 32, 32, 7, 7, 9) is False
    got = ops.conv3d_wgrad_narrow_f16x2_plan(3, 32, 32, 7, 7, 7)
    assert got == dict(zip(("tile_z", "slots", "tiles_per_slot", "chain", "folds"), plan(L, (3, 32, 32, 7, 7, 7))))
    with pytest.raises(m3d.M3DError):
        ops.conv3d_wgrad_narrow_f16x2_plan(3, 32, 32, 7, 7, 9)


GRID = [(b, cin, cout, d, h, w) for b in (1, 4, 300) for cin, cout in ((32, 32), (16, 32), (64, 96), (256, 256), (48, 32))
        for d, h, w in ((7, 7, 7), (7, 7, 8), (7, 7, 9), (4, 9, 1), (16, 16, 16), (2, 4, 16), (64, 64, 64))]


def test_wgrad_kernel_without_the_keyword_is_unchanged(L):
    from m3d import conv_plan as cp
    for s in GRID:
        for mode in ("fp32", "f16x2"):
            for narrow in (False, True):
                for k in (1, 3, 5):
                    assert cp.wgrad_kernel(*s, mode, k=k, narrow=narrow, narrow_f16=None) == cp.wgrad_kernel(*s, mode, k=k, narrow=narrow), s
            assert cp.wgrad_kernel(*s, mode, narrow_f16=None) == cp.wgrad_kernel(*s, mode), s
    with pytest.raises(ValueError):
        cp.wgrad_kernel(1, 32, 32, 7, 7, 7, "bf16", narrow_f16=0)


def test_wgrad_kernel_routes_supported_layers_from_the_threshold(L):
    from m3d import conv_plan as cp
    assert cp.WGRAD_NARROW_F16X2 == "f16x2 narrow" and isinstance(cp.WGRAD_NARROW_F16X2_MIN_WORK, int) and cp.WGRAD_NARROW_F16X2_MIN_WORK > 0
    settings = [(mode, narrow) for mode in ("fp32", "f16x2") for narrow in (False, True)]
    for s in GRID:
        work = s[0] * s[1] * s[2] * s[3] * s[4] * s[5]
        takes = bool(L.m3d_conv3d_wgrad_narrow_f16x2_supported(*s))
        assert takes == (s[5] <= 8 and s[1] % 32 == 0 and s[2] % 32 == 0), s
        for mode, narrow in settings:
            today = cp.wgrad_kernel(*s, mode, narrow=narrow)
            assert today != cp.WGRAD_NARROW_F16X2
            for thr in (0, work):                                                      # at or above the threshold
                got = cp.wgrad_kernel(*s, mode, narrow=narrow, narrow_f16=thr)
                assert got == (cp.WGRAD_NARROW_F16X2 if takes else today), (s, mode, narrow, thr)
            assert cp.wgrad_kernel(*s, mode, narrow=narrow, narrow_f16=work + 1) == today, s       # one product below it
            assert cp.wgrad_kernel(*s, mode, k=1, narrow=narrow, narrow_f16=0) == cp.WGRAD_FP32, s      # k = 1
    for mode, narrow in settings:
        assert cp.wgrad_kernel(4, 32, 32, 7, 7, 9, mode, narrow=narrow, narrow_f16=0) == cp.wgrad_kernel(4, 32, 32, 7, 7, 9, mode, narrow=narrow)
        assert cp.wgrad_kernel(4, 16, 32, 7, 7, 7, mode, narrow=narrow, narrow_f16=0) == cp.wgrad_kernel(4, 16, 32, 7, 7, 7, mode, narrow=narrow)
        assert cp.wgrad_kernel(4, 1, 32, 7, 7, 7, mode, k=5, narrow=narrow, narrow_f16=0) == cp.WGRAD_FP32
    # the default threshold: the constant, in products per tap
    w = cp.WGRAD_NARROW_F16X2_MIN_WORK
    R = -(-w // (343 * 256 * 256))
    assert cp.wgrad_kernel(R, 256, 256, 7, 7, 7, "fp32", narrow_f16=w) == cp.WGRAD_NARROW_F16X2
    if R > 1:
        assert cp.wgrad_kernel(R - 1, 256, 256, 7, 7, 7, "fp32", narrow_f16=w) == cp.WGRAD_FP32


def test_the_plan_passes_the_threshold_on_and_leaves_gy_reduce_and_gb_alone(L):
    from m3d import conv_plan as cp
    x, w = (4, 32, 7, 7, 7), (64, 32, 3, 3, 3)
    for train in ("fp32", "f16x2"):
        for narrow in (None, 0):
            for wg in ("fp32", "f16x2"):
                for wn in (False, True):
                    s = cp.TrainSetting(train=train, min_units=0, narrow=narrow, wgrad=wg, wgrad_narrow=wn)
                    off = cp.plan_train_conv(s, x, w, 1, (True, True, True))
                    assert cp.plan_train_conv(s._replace(wgrad_narrow_f16=None), x, w, 1, (True, True, True)) == off
                    on = cp.plan_train_conv(s._replace(wgrad_narrow_f16=0), x, w, 1, (True, True, True))
                    assert on.wgrad == cp.WGRAD_NARROW_F16X2 and off.wgrad != cp.WGRAD_NARROW_F16X2
                    assert on._replace(wgrad=off.wgrad) == off                          # forward, sweep, dgrad, gy_reduce, gb
                    assert cp.plan_train_conv(s._replace(wgrad_narrow_f16=4 * 32 * 64 * 343 + 1), x, w, 1, (True, True, True)) == off
                    assert cp.plan_train_conv(s._replace(wgrad_narrow_f16=0), x, w, 1, (True, False, True)).wgrad is None
                    assert cp.plan_train_backward(s._replace(wgrad_narrow_f16=0), x, w, 1, (True, True, True)) == tuple(on)[2:]
    d2 = cp.TrainSetting(dilated="m3d")
    assert cp.plan_train_conv(d2._replace(wgrad_narrow_f16=0), x, w, 2, (True, True, True)).wgrad == cp.WGRAD_DILATED


def test_the_switch_round_trips_and_install_leaves_it_off(L):
    import m3d.compat as c
    from m3d import conv_plan as cp
    assert c.get_conv_wgrad_narrow_f16() is False and c._setting.wgrad_narrow_f16 is None          # default off
    try:
        assert c.set_conv_wgrad_narrow_f16(True) is False and c.get_conv_wgrad_narrow_f16() is True
        assert c._setting.wgrad_narrow_f16 == cp.WGRAD_NARROW_F16X2_MIN_WORK                       # min_work=None: the constant
        assert c.get_conv_wgrad_narrow() is False and c.get_conv_wgrad() == "fp32" and c.get_conv_train_narrow() is False
        c.install_conv3d(), c.install_linear()                  # what install() does to F.conv3d / F.linear leaves it alone
        assert c.get_conv_wgrad_narrow_f16() is True
        assert c.set_conv_wgrad_narrow_f16(True, 0) is True and c._setting.wgrad_narrow_f16 == 0   # 0 routes every supported layer
        assert c.set_conv_wgrad_narrow_f16(True) is True and c._setting.wgrad_narrow_f16 == cp.WGRAD_NARROW_F16X2_MIN_WORK
        assert c.set_conv_wgrad_narrow_f16(False) is True and c.get_conv_wgrad_narrow_f16() is False
        with pytest.raises(ValueError):
            c.set_conv_wgrad_narrow_f16(True, -1)
        assert c.get_conv_wgrad_narrow_f16() is False
        # set_conv_wgrad_narrow keeps its meaning and its bool(on)
        assert c.set_conv_wgrad_narrow(1) is False and c.get_conv_wgrad_narrow() is True and c.get_conv_wgrad_narrow_f16() is False
        assert c.set_conv_wgrad_narrow(False) is True
        c.uninstall_conv3d(), c.uninstall_linear()
        c.install()
        assert c.get_conv_wgrad_narrow_f16() is False
    finally:
        c.set_conv_wgrad_narrow_f16(False)
        c.set_conv_wgrad_narrow(False)
        c.uninstall_conv3d(), c.uninstall_linear()
