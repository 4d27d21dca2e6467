"""CPU: the case table of tests/wino_conv_cases.py reaches every production instantiation of the four fp32 Winograd conv kernels under its
conditions - asked of the library's own host queries (m3d_conv3d_wino2_plan, m3d_conv3d_stem_wino_plan), so that a moved threshold fails
here and not silently on the GPU; every integer case is provably exact; the NumPy emulation of the kernels' algorithm is a convolution,
is exact on the integer operands and stays inside the random-data bound; and seeded defects of that emulation are caught by both forms
of the GPU tests' comparison (tests/test_gpu_wino_conv.py)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import wino_conv_cases as T

M3D_EINVAL, M3D_EUNSUPPORTED = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("", "pool", "pool+argmax")
VARIANTS = {
    "w24": [(4, 32, 1, ""), (4, 16, 1, "")] + [(4, 8, ks, "") for ks in (1, 2, 3, 5, 8)] + [(4, t, 1, m) for t in (32, 16) for m in MODES[1:]],
    "w22": [(2, 32, 1, ""), (2, 16, 1, "")] + [(2, 8, ks, "") for ks in (1, 2, 3, 5, 8)],
    "stem": [(pool, planes) for pool in (False, True) for planes in (4, 8)],
    "w23x": ["w48", "w24c64", "w24", "pool"],
}
# the shapes (B, cin, cout, D, H, W) of the 2-D Winograd tests of tests/test_gpu_ops.py, by test
OPS_SHAPES = {
    "test_conv3d_winograd_vs_fp64": [(1, 32, 64, 6, 9, 64), (1, 64, 64, 5, 8, 70), (2, 5, 7, 4, 5, 48), (1, 64, 128, 6, 11, 32), (1, 128, 128, 4, 6, 37),
                                     (1, 33, 40, 3, 4, 24), (1, 16, 96, 7, 13, 129), (1, 256, 256, 3, 25, 25), (1, 2, 200, 2, 3, 100)],
    "test_conv3d_winograd_2d_pool_argmax": [(1, 64, 64, 6, 8, 64), (2, 32, 40, 4, 10, 70), (1, 128, 128, 4, 6, 32), (1, 16, 33, 5, 7, 50)],
    "test_conv3d_winograd_2d_split_k_small_maps": [(1, 128, 256, 16, 16, 16), (1, 256, 256, 8, 25, 23), (2, 20, 40, 3, 13, 12), (1, 256, 70, 5, 9, 17),
                                                   (1, 6, 33, 2, 30, 21)],
    "test_conv3d_winograd_ab_families_agree_with_fp64": [(2, 64, 128, 9, 22, 70)],
    "test_conv3d_winograd_local_family_is_exactly_local": [(1, 64, 64, 4, 16, 128)],
}


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from m3d import ops as _ops
    return _ops


def cdiv(a, b):
    return (a + b - 1) // b


def tiles(c):
    tx, ty, tz, cot, _ = T.tile_of(c)
    return cdiv(c.W, tx), cdiv(c.H, ty), cdiv(c.D, tz), cdiv(c.cout, cot)


def is_ragged(c):
    tx, ty, tz, _, _ = T.tile_of(c)
    return min(tiles(c)[:3]) >= 2 and c.W % tx != 0 and c.H % ty != 0 and c.D % tz != 0


def has_partial_chunk(c):
    cc = T.tile_of(c)[4]
    return c.cin % cc != 0 and cdiv(c.cin, cc) >= 2


def has_partial_cout_tile(c):
    one_tile = c.kernel == "w23x" and c.variant == "w24"              # cout < 64 by its rule: one tile of 64 channels
    return c.cout % 32 != 0 and (tiles(c)[3] >= 2 or (one_tile and cdiv(c.cout, 32) == 2))


def by_variant(cond):
    return {(c.kernel, c.variant) for c in T.CASES if cond(c)}


ALL = {(k, v) for k, vs in VARIANTS.items() for v in vs}


# ------------------------------------------------------------------ plans
def test_every_case_runs_the_variant_it_names(ops):
    from m3d import _lib
    assert len(set(T.CASES)) == len(T.CASES)
    assert ops.lib().m3d_conv3d_wino2_family() == 4
    for c in T.CASES:
        if c.kernel in ("w24", "w22"):
            fam, tile, ks, mode = c.variant
            assert (c.pool, c.argmax) == (mode != "", mode == "pool+argmax") and mode in MODES
            if not c.pool:
                assert ops.conv3d_wino2_plan(c.batch, c.cin, c.cout, c.D, c.H, c.W, local=c.kernel == "w22") == (fam, tile, ks), c
            else:                                                      # forward_pool2: the default family, the tile by width, no K split
                assert c.kernel == "w24" and c.W >= 24 and min(c.D, c.H) >= 2 and (fam, tile, ks) == (4, 16 if c.W < 48 else 32, 1), c
        elif c.kernel == "stem":
            pool, planes = c.variant
            assert pool == c.pool and c.cin == 1 and not c.argmax
            assert ops.conv3d_stem_wino_plan(c.batch, c.cout, c.D, c.H, c.W, c.pool) == 4, c      # the release library at these sizes
            if planes == 8:                                            # reached through the tuning library's option, as the GPU test does
                with _lib.tuning():
                    _lib.set_option("tune_stem", 8)
                    assert ops.conv3d_stem_wino_plan(c.batch, c.cout, c.D, c.H, c.W, c.pool) == 8
        else:
            assert c.variant is not None and c.variant == T.W23X_RULE(c.cout, c.W, c.pool) and not c.argmax, c


def test_every_variant_has_a_case_and_one_lead_case():
    assert {(c.kernel, c.variant) for c in T.CASES} >= ALL
    assert sorted(map(str, ((c.kernel, c.variant) for c in T.LEAD))) == sorted(map(str, ALL))
    extra = {(c.kernel, c.variant) for c in T.CASES} - ALL            # further reachable K splits are welcome, nothing else
    assert all(k in ("w24", "w22") and v[1] == 8 and v[3] == "" for k, v in extra), extra


def test_stem_plan_pins_the_release_choice(ops):
    """eight planes per workgroup only from 1024 workgroups of eight planes on: the 1 x 1 -> 32 stem on 128^3 is 2 * 16 * 16 = 512 of them
    and runs 4 planes; batch 2, or 200 voxels wide, reaches 1024.  The query answers with the launch's own function, so the tuning
    option moves both."""
    from m3d import _lib
    assert ops.conv3d_stem_wino_plan(1, 32, 128, 128, 128) == 4
    assert ops.conv3d_stem_wino_plan(1, 32, 128, 128, 128, pool=True) == 4
    assert ops.conv3d_stem_wino_plan(2, 32, 128, 128, 128) == 8
    assert ops.conv3d_stem_wino_plan(1, 32, 128, 128, 200) == 8
    assert ops.conv3d_stem_wino_plan(1, 33, 128, 128, 128) == 8          # two cout tiles
    assert ops.conv3d_stem_wino_plan(1, 32, 120, 128, 200) == 4          # 15 * 16 * 4 = 960
    for c in T.CASES:
        if c.kernel == "stem":
            assert ops.conv3d_stem_wino_plan(c.batch, c.cout, c.D, c.H, c.W, c.pool) == 4
    with _lib.tuning():
        _lib.set_option("tune_stem", 8)
        assert ops.conv3d_stem_wino_plan(1, 32, 16, 16, 64) == 8
        _lib.set_option("tune_stem", 4)
        assert ops.conv3d_stem_wino_plan(2, 32, 128, 128, 128) == 4
    assert ops.conv3d_stem_wino_plan(2, 32, 128, 128, 128) == 8


def test_stem_plan_refuses_what_the_launch_refuses(ops):
    L = ops.lib()

    def rc_of(*a):
        p = C.c_int(-1)
        rc = L.m3d_conv3d_stem_wino_plan(*a, C.byref(p))
        assert (rc == 0) == (p.value in (4, 8)) and (rc == 0 or p.value == -1)
        return rc
    assert rc_of(1, 32, 8, 8, 31, 0) == M3D_EUNSUPPORTED                  # narrower than 32: the direct stem kernel's maps
    assert rc_of(1, 32, 8, 8, 32, 0) == 0
    assert rc_of(65536, 32, 8, 8, 32, 0) == M3D_EUNSUPPORTED              # batch is a grid dimension
    assert rc_of(1, 32, 1024, 1024, 512, 0) == M3D_EUNSUPPORTED           # one item no longer fits 32-bit byte offsets
    assert rc_of(1, 32, 1, 8, 32, 1) == M3D_EINVAL and rc_of(1, 32, 8, 1, 32, 1) == M3D_EINVAL and rc_of(1, 32, 1, 1, 32, 0) == 0
    for bad in ((0, 32, 8, 8, 32), (1, 0, 8, 8, 32), (1, 32, 0, 8, 32), (1, 32, 8, -1, 32), (1, 32, 8, 8, 0)):
        assert rc_of(*bad, 0) == M3D_EINVAL
    assert L.m3d_conv3d_stem_wino_plan(1, 32, 8, 8, 32, 0, None) == 0     # the output is optional
    assert ops.conv3d_stem_wino_plan(1, 32, 8, 8, 31) is None


# ------------------------------------------------------------------ conditions
def test_ragged_tiles():
    assert by_variant(is_ragged) >= ALL


def test_odd_cin_and_partial_chunks():
    stem = {(k, v) for k, v in ALL if k == "stem"}
    assert by_variant(lambda c: has_partial_chunk(c) and c.cin % 2 == 1) >= ALL - stem
    assert all(c.cin == 1 for c in T.CASES if c.kernel == "stem")


def test_partial_cout_tiles_and_odd_block_counts():
    assert by_variant(has_partial_cout_tile) >= ALL
    for kernel in VARIANTS:
        assert any(c.kernel == kernel and cdiv(c.cout, 32) % 2 == 1 and cdiv(c.cout, 32) >= 3 for c in T.CASES), kernel


def test_batch_two():
    assert by_variant(lambda c: c.batch == 2) >= ALL


def test_lead_cases_hold_every_condition():
    for c in T.LEAD:
        assert is_ragged(c) and has_partial_cout_tile(c) and c.batch == 2, c
        assert c.kernel == "stem" or (has_partial_chunk(c) and c.cin % 2 == 1), c
        if c.pool:                                  # the pool drops the last plane, row and column of an odd volume
            assert c.D % 2 == 1 and c.H % 2 == 1, c


def test_every_width_residue_on_every_2d_tile():
    for kernel, fam in (("w24", 4), ("w22", 2)):
        for tile in (32, 16, 8):
            res = {c.W % 4 for c in T.CASES if c.kernel == kernel and c.variant[1] == tile and not c.pool}
            assert res == {0, 1, 2, 3}, (kernel, tile, res)
    assert {c.W % 2 for c in T.CASES if c.pool and c.kernel == "w24"} == {0, 1}
    assert {(c.W // 2) % 2 for c in T.CASES if c.pool and c.kernel == "w24"} == {0, 1}      # pooled rows stored in pairs and one by one
    for kernel in ("stem", "w23x"):
        assert {c.W % 2 for c in T.CASES if c.kernel == kernel and not c.pool} == {0, 1}, kernel


def test_tile_order_edges():
    for kernel in ("w24", "w22"):
        mine = [c for c in T.CASES if c.kernel == kernel]
        grids = [int(np.prod(tiles(c))) for c in mine]
        assert any(g % 8 != 0 and g > 8 for g in grids), kernel                      # the XCD remap's remainder
        assert any(tiles(c)[2] >= 5 and tiles(c)[2] % 4 != 0 and tiles(c)[1] >= 2 for c in mine), kernel     # z groups of four + a remainder group
    assert any(c.kernel == "w24" and tiles(c)[0] > 16 for c in T.CASES)              # the x-slow order
    assert any(c.kernel == "w24" and 1 < tiles(c)[0] <= 16 for c in T.CASES)


def test_k_splits_and_the_short_last_slice():
    for kernel in ("w24", "w22"):
        mine = [c for c in T.CASES if c.kernel == kernel and c.variant[1] == 8]
        assert {c.variant[2] for c in mine} >= {1, 2, 3, 5, 8}, kernel
        five = [c for c in mine if c.variant[2] == 5]
        assert any(c.cin == 33 and [len(s) for s in T.slices_of(c)] == [8, 8, 8, 8, 1] for c in five), kernel
        assert any(np.prod(tiles(c)) * c.batch == 1 for c in mine), kernel           # a single tile
        for c in mine:
            sl = T.slices_of(c)
            assert len(sl) == c.variant[2] and [ci for s in sl for ci in s] == list(range(c.cin))
    c = next(c for c in T.LEAD if c.kernel == "w23x" and c.variant == "w24")
    assert T.slices_of(c) == [[0, 1, 4, 5], [2, 3, 6]]


def test_cost_cap():
    for c in T.CASES:
        assert T.flop(c) <= T.CAP_FLOP, (c, T.flop(c))


def test_the_older_tests_miss_plans_this_table_reaches(ops):
    """The finding this table answers, kept visible: the shapes of test_gpu_ops.py's 2-D Winograd tests are small maps that the library
    runs on other instantiations than the workload's - under the default family all but two plan to the K-split 16x16x2 tile."""
    src = open(os.path.join(ROOT, "tests", "test_gpu_ops.py")).read()
    shapes = []
    for name, ss in OPS_SHAPES.items():
        assert ("def %s(" % name) in src
        for s in ss:
            assert str(s) in src or name in ("test_conv3d_winograd_ab_families_agree_with_fp64", "test_conv3d_winograd_local_family_is_exactly_local"), (name, s)
            shapes.append(s)
    assert len(shapes) == 20
    old4 = [ops.conv3d_wino2_plan(*s) for s in shapes]
    old2 = [ops.conv3d_wino2_plan(*s, local=True) for s in shapes]
    new4 = {c.variant[:3] for c in T.CASES if c.kernel == "w24" and not c.pool}
    new2 = {c.variant[:3] for c in T.CASES if c.kernel == "w22"}
    assert sum(p[1] == 8 for p in old4) == 18 and sum(p == (4, 32, 1) for p in old4) == 2
    assert {p[2] for p in old4 if p[1] == 8} == {2, 4, 5, 8}
    assert sum(p == (2, 16, 1) for p in old2) == 1 and sum(p == (2, 32, 1) for p in old2) == 1
    assert new4 - set(old4) >= {(4, 16, 1), (4, 8, 1), (4, 8, 3)}
    assert new2 - set(old2) >= {(2, 8, 1), (2, 8, 3)}
    assert new4 >= set(old4) and new2 >= set(old2)


# ------------------------------------------------------------------ references (computed once per case)
@functools.lru_cache(maxsize=None)
def ints(c):
    x, w = T.integer_operands(c)
    return x, w, T.conv64(x, w, T.KSIZE[c.kernel])


@functools.lru_cache(maxsize=None)
def rands(c):
    x, w, scale, shift = T.random_operands(c)
    y = T.conv64(x, w, T.KSIZE[c.kernel])
    return x, w, scale, shift, y, T.wino_abs(c, x, w)


def shapes_once(cases):
    """one case per (kernel, emulated algorithm, shape): pooled / arg-max / plane-count variants of one shape share their emulation"""
    seen, out = set(), []
    for c in cases:
        key = (c.kernel, str(T.slices_of(c)), c.batch, c.cin, c.cout, c.D, c.H, c.W)
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_integer_operands_are_provably_exact(c):
    x, w, ref = ints(c)
    xm, wm = T.int_ranges(c)
    assert float(x.abs().max()) <= xm and float(w.abs().max()) <= wm * T.UNIT[c.kernel]
    assert bool((x == x.round()).all()) and bool((w % T.UNIT[c.kernel] == 0).all())
    assert bool((x[:, 0, 0, 0, 0] != 0).all()) and bool((x[:, -1, -1, -1, -1] != 0).all()) and float(w.view(-1)[0]) != 0 != float(w.view(-1)[-1])
    wabs = T.wino_abs(c, x, w)
    assert float(wabs.max()) < 2.0 ** 24 and 4.0 * float(wabs.max()) + 8 < 2.0 ** 23
    assert bool((wabs >= ref.abs()).all())
    u = T.packed_weights(c, w, np.float32)                               # the recipe's claim: every transformed weight an integer
    assert np.array_equal(u, np.round(u)) and np.array_equal(u.astype(np.float64), T.packed_weights(c, w, np.float64))


@pytest.mark.parametrize("c", shapes_once(T.CASES), ids=T.case_id)
def test_emulation_is_a_convolution(c):
    """at fp64, on the random operands: transforms, patch alignment and wino_abs describe the conv (1e-12 of wino_abs, element by element)"""
    x, w, scale, shift, y, wabs = rands(c)
    assert bool(((T.emulate(c, x, w, dtype=np.float64) - y).abs() <= 1e-12 * wabs).all())
    assert bool(((T.wino_plain(c, x, w) - y).abs() <= 1e-12 * wabs).all())
    assert bool((wabs >= y.abs()).all())


@pytest.mark.parametrize("c", shapes_once(T.CASES), ids=T.case_id)
def test_emulation_is_exact_on_the_integer_operands(c):
    x, w, ref = ints(c)
    assert torch.equal(T.emulate(c, x, w).to(T.F64), ref)
    scale, shift = T.epilogue_operands(c, negative=c.kernel == "stem")
    assert torch.equal(T.emulate(c, x, w, scale=scale, shift=shift, relu=True).to(T.F64), T.epilogue64(ref, scale, shift))


WORST = {}


@pytest.mark.parametrize("c", shapes_once(T.CASES), ids=T.case_id)
def test_emulation_stays_inside_the_random_data_bound(c):
    x, w, scale, shift, y, wabs = rands(c)
    r1 = float(((T.emulate(c, x, w).to(T.F64) - y).abs() / T.bound(c, y, wabs)).max())
    ye = T.epilogue64(y, scale, shift)
    r2 = float(((T.emulate(c, x, w, scale=scale, shift=shift, relu=True).to(T.F64) - ye).abs() / T.bound(c, ye, wabs, scale, shift)).max())
    WORST[c.kernel] = max(WORST.get(c.kernel, 0.0), r1, r2)
    print("wino emulation ratio: %s plain %.4f epilogue %.4f (worst of %s so far %.4f)" % (T.case_id(c), r1, r2, c.kernel, WORST[c.kernel]))
    assert r1 <= 1.0 and r2 <= 1.0, (T.case_id(c), r1, r2)


# ------------------------------------------------------------------ the tests can fail
def defective(c, defect, x, w, scale, shift):
    """the emulation with one seeded defect and the reference it is held against (shift_per_slice shows in the epilogue only)"""
    if defect == "shift_per_slice":
        return T.emulate(c, x, w, scale=scale, shift=shift, relu=False, defect=defect).to(T.F64), True
    return T.emulate(c, x, w, defect=defect).to(T.F64), False


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_seeded_defects_break_exact_equality(defect):
    """on every case the defect applies to: the integer operands expose it"""
    hit = 0
    for c in shapes_once(T.CASES):
        if not T.defect_applies(c, defect):
            continue
        x, w, ref = ints(c)
        scale, shift = T.epilogue_operands(c)
        got, epi = defective(c, defect, x, w, scale, shift)
        want = T.epilogue64(ref, scale, shift, relu=False) if epi else ref
        assert not torch.equal(got, want), (defect, T.case_id(c))
        hit += 1
    assert hit >= 4, (defect, hit)


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_seeded_defects_exceed_the_random_data_bound(defect):
    """on every LEAD case the defect applies to, at least one element leaves the bound"""
    kernels = set()
    for c in shapes_once(T.LEAD):
        if not T.defect_applies(c, defect):
            continue
        x, w, scale, shift, y, wabs = rands(c)
        got, epi = defective(c, defect, x, w, scale, shift)
        if epi:
            want = T.epilogue64(y, scale, shift, relu=False)
            ratio = float(((got - want).abs() / T.bound(c, want, wabs, scale, shift)).max())
        else:
            ratio = float(((got - y).abs() / T.bound(c, y, wabs)).max())
        assert ratio > 1.0, (defect, T.case_id(c), ratio)
        kernels.add(c.kernel)
    want_kernels = {"coef5": {"w24", "stem"}, "short_slice": {"w24", "w22", "w23x"}, "shift_per_slice": {"w24", "w22"}}
    assert kernels == want_kernels.get(defect, set(VARIANTS)), (defect, kernels)
