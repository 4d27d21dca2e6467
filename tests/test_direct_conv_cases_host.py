"""CPU: the case table of tests/direct_conv_cases.py reaches every production instantiation of the direct fp32 conv, each at a ragged
volume, an odd cin with a partial chunk, a half-empty cout tile and batch 2 - asked of the library's own host query
(m3d_conv3d_direct_plan), so that a moved dispatcher threshold fails here and not silently on the GPU."""
import ctypes as C

import pytest

import direct_conv_cases as T

M3D_EINVAL, M3D_EUNSUPPORTED = -1, -4
NAMES = ("variant", "cc", "tile_x", "tile_y", "tile_z", "ncb", "ksplit")
# template arguments <CC, XB, ROWS, NCB, KS> -> (cc, tile_x, tile_y, tile_z, ncb, ksplit) of every variant: the tile of a workgroup of
# 4 waves stacked along z is XB x (ROWS * 32 / XB) x 4 voxels (the pool variants: 2 x 2 waves of 2 x 2 rows)
VARIANTS = {
    0: (4, 32, 4, 4, 1, 1), 1: (4, 16, 4, 4, 1, 1), 2: (4, 8, 8, 4, 1, 1),
    3: (2, 32, 4, 4, 2, 1), 4: (8, 32, 2, 4, 2, 2), 5: (8, 32, 1, 4, 2, 2), 6: (2, 32, 2, 4, 2, 1), 7: (4, 32, 1, 4, 2, 1),
    8: (4, 16, 4, 4, 2, 1), 9: (4, 16, 2, 4, 1, 1), 10: (8, 16, 2, 4, 1, 2), 11: (4, 8, 8, 4, 2, 1), 12: (4, 8, 4, 4, 1, 1),
    13: (2, 32, 4, 4, 2, 1),
    14: (32, 32, 1, 4, 2, 1), 15: (32, 16, 2, 4, 2, 1), 16: (32, 8, 4, 4, 2, 1),
    17: (1, 32, 4, 4, 1, 1), 18: (1, 32, 4, 4, 1, 1), 19: (1, 32, 4, 4, 2, 1),
}
ONE_COUT_TILE = (0, 1, 2, 17, 18, 19)      # cout <= 32 (ncb_total == 1), and the stem: all of its <= 32 * ncb channels in one workgroup


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import LIB_PATH
    return C.CDLL(LIB_PATH)


def plan(L, c):
    out = [C.c_int(-1) for _ in NAMES]
    rc = L.m3d_conv3d_direct_plan(c.batch, c.cin, c.cout, c.D, c.H, c.W, c.k, int(c.pool), *[C.byref(v) for v in out])
    return rc, dict(zip(NAMES, (v.value for v in out)))


@pytest.fixture(scope="module")
def plans(L):
    out = {}
    for c in T.CASES:
        rc, p = plan(L, c)
        assert rc == 0, (c, rc)
        out[c] = p
    return out


def cdiv(a, b):
    return (a + b - 1) // b


def is_ragged(c, p):
    tiles = (cdiv(c.D, p["tile_z"]), cdiv(c.H, p["tile_y"]), cdiv(c.W, p["tile_x"]))
    return (min(tiles) >= 2 and c.D % p["tile_z"] != 0 and c.W % p["tile_x"] != 0 and (p["tile_y"] == 1 or c.H % p["tile_y"] != 0))


def has_partial_chunk(c, p):
    return c.cin % 2 == 1 and c.cin % p["cc"] != 0 and cdiv(c.cin, p["cc"]) >= 2


def has_half_empty_cout_tile(c, p):
    per = 32 * p["ncb"]
    return c.cout % per != 0 and (p["variant"] in ONE_COUT_TILE or cdiv(c.cout, per) >= 2)


def covered(plans, cond):
    return {p["variant"] for c, p in plans.items() if cond(c, p)}


def test_every_case_runs_the_variant_it_names(plans):
    for c, p in plans.items():
        assert p["variant"] == c.variant, (c, p)
        assert tuple(p[n] for n in NAMES[1:]) == VARIANTS[c.variant], (c, p)
    assert len(set(T.CASES)) == len(T.CASES)
    assert {c.variant for c in T.LEAD} == set(VARIANTS) and len(T.LEAD) == len(VARIANTS)


def test_every_variant_is_covered(L, plans):
    count = L.m3d_conv3d_direct_plan_count()
    assert count == len(VARIANTS)
    assert sorted({p["variant"] for p in plans.values()}) == list(range(count))


def test_ragged_tiles(L, plans):
    assert covered(plans, is_ragged) == set(range(L.m3d_conv3d_direct_plan_count()))


def test_odd_cin_and_partial_chunks(L, plans):
    """the 5^3 stem is exempt: its single input channel has no chunks (its K index is the tap; 125 taps = 62 pairs + a half-empty one)"""
    stem = {p["variant"] for c, p in plans.items() if c.k == 5}
    assert stem == {17, 18, 19}
    assert covered(plans, has_partial_chunk) == set(range(L.m3d_conv3d_direct_plan_count())) - stem
    for c, p in plans.items():
        if c.k == 5:
            assert c.cin == 1


def test_half_empty_cout_tiles(L, plans):
    assert covered(plans, has_half_empty_cout_tile) == set(range(L.m3d_conv3d_direct_plan_count()))
    for c, p in plans.items():                      # the variants listed as single-tile really cannot have a second cout tile
        if p["variant"] in ONE_COUT_TILE:
            assert c.cout <= 32 * p["ncb"]


def test_batch_two(L, plans):
    assert covered(plans, lambda c, p: c.batch == 2) == set(range(L.m3d_conv3d_direct_plan_count()))


def test_one_lead_case_per_variant_holds_every_condition(plans):
    for c in T.LEAD:
        p = plans[c]
        assert is_ragged(c, p) and has_half_empty_cout_tile(c, p) and c.batch == 2, c
        assert c.k == 5 or has_partial_chunk(c, p), c


def test_cost_cap(plans):
    for c in T.CASES:
        assert T.flop(c) <= T.CAP_FLOP, (c, T.flop(c))
    for c in T.LEAD:                                # the pool drops the last plane, row and column of an odd volume
        if c.pool:
            assert c.D % 2 == 1 and c.H % 2 == 1 and c.W % 2 == 1, c


def test_k1_and_stem_thresholds(L):
    """the k = 1 variants by width (>= 24, 12..23, < 12), the stem variants by cout and pool - on both sides of every threshold"""
    for w, v in ((40, 14), (24, 14), (23, 15), (12, 15), (11, 16), (1, 16)):
        rc, p = plan(L, T.Case(v, 1, 8, 8, 3, 3, w, 1, False))
        assert (rc, p["variant"]) == (0, v), w
    for cout, pool, v in ((1, False, 18), (32, False, 18), (33, False, 19), (64, False, 19), (1, True, 17), (32, True, 17)):
        rc, p = plan(L, T.Case(v, 1, 1, cout, 5, 5, 9, 5, pool))
        assert (rc, p["variant"]) == (0, v), (cout, pool)


def test_plan_refuses_what_the_dispatcher_refuses(L):
    """M3D_EUNSUPPORTED / M3D_EINVAL exactly where conv_dispatch returns them, and no output is written then"""
    def rc_of(batch, cin, cout, D, H, W, k, pool):
        rc, p = plan(L, T.Case(-1, batch, cin, cout, D, H, W, k, pool))
        assert rc == 0 or all(v == -1 for v in p.values()), p
        return rc
    assert rc_of(1, 1, 65, 8, 8, 8, 5, False) == M3D_EUNSUPPORTED         # stem: more than 64 channels
    assert rc_of(1, 2, 32, 8, 8, 8, 5, False) == M3D_EUNSUPPORTED         # k = 5 with cin != 1
    assert rc_of(1, 1, 33, 8, 8, 8, 5, True) == M3D_EUNSUPPORTED          # stem + pool: one cout block only
    assert rc_of(1, 8, 8, 8, 8, 23, 3, True) == M3D_EUNSUPPORTED          # k = 3 + pool: maps >= 24 wide
    assert rc_of(1, 8, 8, 8, 8, 24, 3, True) == 0
    assert rc_of(1, 8, 8, 8, 8, 32, 1, True) == M3D_EUNSUPPORTED          # k = 1 has no pool
    assert rc_of(1, 8, 8, 8, 8, 32, 7, False) == M3D_EUNSUPPORTED
    assert rc_of(65536, 8, 8, 2, 2, 8, 3, False) == M3D_EUNSUPPORTED      # batch is a grid dimension
    assert rc_of(65535, 8, 8, 2, 2, 8, 3, False) == 0
    assert rc_of(1, 8, 8, 512, 512, 256, 3, False) == M3D_EUNSUPPORTED    # 32 channels of one item no longer fit int offsets
    assert rc_of(1, 8, 8, 512, 512, 255, 3, False) == 0
    for bad in ((0, 8, 8, 4, 4, 4), (1, 0, 8, 4, 4, 4), (1, 8, 0, 4, 4, 4), (1, 8, 8, 0, 4, 4), (1, 8, 8, 4, -1, 4), (1, 8, 8, 4, 4, 0)):
        assert rc_of(*bad, 3, False) == M3D_EINVAL
    assert L.m3d_conv3d_direct_plan(1, 8, 8, 4, 4, 4, 3, 0, None, None, None, None, None, None, None) == 0     # outputs are optional


def test_plan_ignores_the_tuning_override(L):
    """the query names the production choice; tune_k3 of the tuning build overrides launches only.  No device call."""
    from m3d import _lib, ops
    c = T.LEAD[3]
    with _lib.tuning():
        _lib.set_option("tune_k3", 36)
        assert ops.conv3d_direct_plan(c.batch, c.cin, c.cout, c.D, c.H, c.W)["variant"] == 3
    assert ops.conv3d_direct_plan(c.batch, c.cin, c.cout, c.D, c.H, c.W, c.k, c.pool) == dict(zip(NAMES, (3,) + VARIANTS[3]))
    assert ops.conv3d_direct_plan(1, 8, 8, 8, 8, 23, 3, True) is None


def test_gradient_cases_cover_the_wgrad_edges():
    """the shapes section (c) of the GPU tests relies on, checked here so that an edit of the table cannot drop one"""
    k3 = [c for c in T.WGRAD_CASES if c[6] == 3]
    assert {c[5] % 4 for c in k3} == {0, 1, 2, 3} and {3, 6, 9} <= {c[5] for c in k3}
    assert any(c[4] < 4 for c in k3) and any(c[3] == 1 for c in k3) and any(c[0] == 3 for c in k3)
    assert any(c[1] == 33 for c in k3) and any(c[2] == 70 for c in k3) and any(c[1] == 70 for c in k3) and any(c[2] == 33 for c in k3)
    tiles = [c[0] * cdiv(c[3], 2) * cdiv(c[4], 4) * cdiv(c[5], 16) for c in k3]
    assert min(tiles) == 1 and max(tiles) >= 200
    assert sum(c[6] == 1 for c in T.WGRAD_CASES) >= 1
    assert {c[2] for c in T.WGRAD_CASES if c[6] == 5} == {20, 48} and all(c[1] == 1 for c in T.WGRAD_CASES if c[6] == 5)
    for b, cin, cout, d, h, w, k in T.WGRAD_CASES:        # |x|, |gy| <= 3: every fp32 order of the sum over voxels is exact
        assert 9 * b * d * h * w < 2 ** 24
    for b, ch, d, h, w in T.STEM_DGRAD_CASES:
        assert b == 2 and cdiv(w, 32) >= 2 and cdiv(h, 16) >= 2 and cdiv(d, 8) >= 2 and w % 32 and h % 16 and d % 8
    assert {c[1] for c in T.STEM_DGRAD_CASES} == {20, 48}
