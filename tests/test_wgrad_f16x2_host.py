"""The f16x2 conv weight gradient on the CPU (tests/wgrad_f16x2_contract.py): the exact emulation of the cut meets the per-element bound on
every case and input family, each mutant of the cut breaks it somewhere, the library's plan gives the case list the coverage it claims,
and the C entry points refuse what they document - before any pointer is followed (the pointers handed over here lead nowhere)."""
import ctypes as C
import random

import pytest
import torch

import wgrad_f16x2_contract as K


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


def plan(L, case):
    v = [C.c_int(0) for _ in range(4)]
    assert L.m3d_conv3d_wgrad_f16x2_plan(*case, *[C.byref(a) for a in v]) == 0, case
    return tuple(a.value for a in v)              # slots, tiles_per_slot, chain, folds


def check(got, y, E):
    return bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


@pytest.mark.parametrize("relu_x", [False, True], ids=["signed_x", "relu_x"])
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("name", sorted(K.CASES))
def test_cut_meets_the_bound(L, name, family, relu_x):
    case = K.CASES[name]
    _, _, chain, folds = plan(L, case)
    gy, x = K.make_inputs(family, case, 5, relu_x)
    y, E, Cm, A, B = K.contract(gy, x, chain + folds)
    got = K.emulate(K.wgrad_op, gy, x, A, B)
    assert check(got, y, E)
    assert bool((got[Cm == 0] == 0).all())
    if family == "zero":
        assert bool((got == 0).all()) and bool((E == 0).all())


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_every_mutant_breaks_the_bound_somewhere(L, mutant):
    """a bound no mutant violates has no teeth: each mutant of the cut leaves it on at least one of MUTANT_CASES x families.  On its own
    inputs, so it holds under any selection or order of the tests"""
    broke = []
    for name in K.MUTANT_CASES:
        case = K.CASES[name]
        _, _, chain, folds = plan(L, case)
        for family in K.FAMILIES:
            for relu_x in (False, True):
                gy, x = K.make_inputs(family, case, 5, relu_x)
                y, E, _, A, B = K.contract(gy, x, chain + folds)
                assert check(K.emulate(K.wgrad_op, gy, x, A, B), y, E)              # the true cut holds on these very inputs
                if not check(K.emulate(K.wgrad_op, gy, x, A, B, mutant), y, E):
                    broke.append((name, family, relu_x))
    assert broke, mutant


def test_plan_gives_the_case_list_its_coverage(L):
    """the coverage rule of the GPU test, proved on the library's own plan: a moved tile size or slot rule fails here"""
    P = {n: plan(L, c) for n, c in K.CASES.items()}
    for n, c in K.CASES.items():
        slots, tps, chain, folds = P[n]
        assert (slots, tps) == K.expected_plan(c), n
        assert chain == tps * K.ROWS_PRODUCTS and 0 < chain <= K.CHAIN_MAX, n
        assert folds == (slots + 7) // 8 + 7 + 2, n
        assert K.flops(c) <= 1.5e9, n
    tz, ty, tx = K.TILE
    B, _, _, D, H, W = K.CASES["ragged3"]
    assert B == 1 and D > tz and D % tz and H > ty and H % ty and W > tx and W % tx          # >= 2 tiles and a ragged last tile per axis
    assert P["ragged3"][0] >= 3 * 8                                                           # every reduce group adds >= 3 partials
    assert P["one_tile"][:2] == (1, 1)                                                        # a single slot
    assert K.CASES["d1_w1"][3] == 1 and K.CASES["hsmall_w2"][4] < ty
    assert sorted({c[5] % 8 for c in K.CASES.values()}) == list(range(8))                     # W % 8 = 0 .. 7
    assert {c[0] for c in K.CASES.values()} >= {1, 2, 3, 5}
    assert {(c[2] // 32, c[1] // 32) for c in K.CASES.values()} >= {(2, 1), (1, 3), (3, 2)}    # 64 <- 32, 32 <- 96, 96 <- 64
    assert P["slot2"][1] == 2 and P["slot2"][0] > 16                                          # several tiles per workgroup
    s16, t16 = P["slot16"][:2]
    assert t16 == 16 and P["slot16"][2] == 384 and s16 >= 3                                   # the full chain; an output folds >= twice
    B, _, _, D, H, W = K.CASES["slot16"]
    assert 0 < (B * ((D + tz - 1) // tz) * ((H + ty - 1) // ty) * ((W + tx - 1) // tx)) % 16 < 16          # a short last slot
    assert K.CASES["roi7_b5"][0] == 5 and K.CASES["roi7_b5"][3:] == (7, 7, 7)


def test_chain_limit_on_the_training_shapes(L):
    """every map of the DSN body at stride 4 and 8 for tiles of 64 x 256 x 256 and 128^3, batch 1 and 4, and the mask head's RoI maps"""
    shapes = []
    for tile in ((64, 256, 256), (128, 128, 128)):
        for lvl, ch in ((1, 32), (2, 64), (3, 128)):                        # m3d.train.DsnBody: conv2a / 2b, 3a / 3b, 4a / 4b (stride 8)
            d, h, w = (t >> lvl for t in tile)
            for batch in (1, 4):
                shapes += [(batch, ch, 2 * ch, d, h, w), (batch, 2 * ch, 2 * ch, d, h, w)]
    shapes += [(r, 256, 256, 7, 7, 7) for r in (1, 5, 64, 512)]
    for s in shapes:
        assert L.m3d_conv3d_wgrad_f16x2_supported(*s) == 1, s
        slots, tps, chain, folds = plan(L, s)
        assert 0 < chain <= K.CHAIN_MAX and chain == tps * K.ROWS_PRODUCTS and slots >= 1, s
        ws = L.m3d_conv3d_wgrad_f16x2_workspace_bytes(*s)
        assert ws == slots * s[1] * s[2] * 27 * 4, s


def test_supported_agrees_with_the_documented_rule(L):
    rnd = random.Random(7)
    for _ in range(2000):
        s = (rnd.choice([0, 1, 2, 5]), rnd.choice([0, 16, 32, 48, 64, 96, 100, 256, 4096, 4128]), rnd.choice([-32, 8, 32, 64, 80, 96, 4096, 8192]),
             rnd.choice([0, 1, 2, 7, 65, 1 << 16]), rnd.choice([-1, 1, 3, 4, 7, 130, 1 << 16]), rnd.choice([0, 1, 7, 15, 16, 17, 255, 1 << 16]))
        ok = K.supported_rule(*s)
        assert bool(L.m3d_conv3d_wgrad_f16x2_supported(*s)) == ok, s
        assert (L.m3d_conv3d_wgrad_f16x2_workspace_bytes(*s) > 0) == ok, s
        rc = L.m3d_conv3d_wgrad_f16x2_plan(*s, None, None, None, None)
        assert rc == (0 if ok else -1 if min(s) < 1 else -4), s
    assert not L.m3d_conv3d_wgrad_f16x2_supported(1, 32, 32, 1 << 20, 1 << 10, 1 << 10)        # 2^32 tiles
    assert L.m3d_conv3d_wgrad_f16x2_supported(4, 256, 256, 128, 128, 128)


def test_every_refusal(L):
    """M3D_EINVAL -1 / M3D_EUNSUPPORTED -4, each before a pointer is followed or anything is launched"""
    p = lambda a: C.c_void_p(a)
    good = dict(x=p(0x10000), gy=p(0x20000), dw=p(0x30000), xm=p(0x40000), gm=p(0x50000), ws=p(0x60000))
    shape = (1, 32, 32, 2, 4, 16)
    need = L.m3d_conv3d_wgrad_f16x2_workspace_bytes(*shape)
    assert need == 32 * 32 * 27 * 4

    def call(shape=shape, ws_bytes=need, **over):
        a = dict(good, **over)
        return L.m3d_conv3d_wgrad_f16x2(a["x"], a["gy"], a["dw"], *shape, a["xm"], a["gm"], a["ws"], C.c_size_t(ws_bytes), None)

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
    for s in ((1, 16, 32, 2, 4, 16), (1, 32, 48, 2, 4, 16), (1, 8192, 32, 2, 4, 16), (1, 32, 32, 1 << 20, 1 << 10, 1 << 10)):
        assert call(shape=s, ws_bytes=1 << 40) == -4, s                    # what `supported` rejects
    assert call(shape=(1, 16, 32, 2, 4, 16), x=None) == -1                 # EINVAL goes first


def test_wgrad_kernel_is_the_routing_rule(L):
    from m3d import conv_plan as cp
    assert cp.wgrad_kernel(1, 64, 64, 64, 64, 64, "fp32") == cp.WGRAD_FP32
    assert cp.wgrad_kernel(1, 16, 32, 64, 64, 64, "f16x2") == cp.WGRAD_FP32          # cin 16
    assert cp.wgrad_kernel(1, 64, 64, 64, 64, 64, "f16x2", k=1) == cp.WGRAD_FP32     # k = 1
    assert cp.wgrad_kernel(1, 1, 32, 64, 64, 64, "f16x2", k=5) == cp.WGRAD_FP32      # the stem
    assert cp.wgrad_kernel(1, 64, 64, 64, 64, 64, "f16x2") == cp.WGRAD_F16X2
    assert cp.wgrad_kernel(1, 128, 256, 16, 16, 16, "f16x2") == cp.WGRAD_F16X2       # the smallest layer measured to win
    assert cp.wgrad_kernel(1, 32, 32, 2, 4, 16, "f16x2") == cp.WGRAD_FP32            # one voxel tile: supported, not routed
    for s in ((1, 32, 64, 64, 64, 64), (4, 256, 256, 16, 16, 16), (1, 64, 64, 32, 128, 128), (1, 128, 128, 16, 64, 64)):
        assert cp.wgrad_kernel(*s, "f16x2") == cp.WGRAD_F16X2, s                     # layers of both training bodies
    with pytest.raises(ValueError):
        cp.wgrad_kernel(1, 64, 64, 64, 64, 64, "bf16")
    import m3d.compat as compat
    assert compat.get_conv_wgrad() == "fp32"
    with pytest.raises(ValueError):
        compat.set_conv_wgrad("f16")
    assert compat.set_conv_wgrad("f16x2") == "fp32" and compat.set_conv_wgrad("fp32") == "f16x2"
