"""CPU: the case table of tests/linear_cases.py reaches every forward linear GEMM instance of csrc/fc_gemm.hip under its coverage conditions -
checked against a Python restatement of the planners AND against the library's own host query m3d_linear_plan, so that a retuned cost model
that moves a case off its instance fails here and not silently on the GPU; every integer case is provably exact (the planes sum to the
operands, the dropped products are zero, sum |x w| < 2^24, and the fp32 emulation equals fp64); every seeded defect of the emulation is
caught by the GPU test's comparison on at least one case; and the fp32 emulation stays inside the random-data bound."""
import functools
import math

import numpy as np
import pytest

import linear_cases as T


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as g
    g.build()
    from m3d import ops as _ops
    return _ops


def cdiv(a, b):
    return (a + b - 1) // b


# ------------------------------------------------------------------ the planners of csrc/fc_gemm.hip, restated (o: the tuning options)
def make_plan(M, N, K, o):
    """-> (slices, slices_tail, full row tiles) of m3d_linear_forward"""
    mt, nt, chunks = cdiv(M, 128), cdiv(N, 128), cdiv(K, 32)
    rem_blocks = cdiv(M - (mt - 1) * 128, 32)
    mt_full = mt - 1 if rem_blocks <= 2 else mt
    tail_cost = 0.45 if rem_blocks == 1 else 0.6
    slots, flop, rate = 64.0, 2.0 * 128 * 128 * float(K), 1.25e14 / 512.0
    ntail = (mt - mt_full) * nt
    smax = min(chunks // 4 + 1, 64)
    nlong = mt_full * nt if mt_full else ntail
    best, bs = 1e30, 1
    for s in range(1, smax + 1):
        rounds = math.ceil(math.ceil(float(nlong) * s / 8.0) / slots)
        t = rounds * (1.0 if mt_full else tail_cost) * flop / s / rate + rounds * 4e-6
        if s > 1:
            t += float(s) * M * N * 8.0 / 4e12 + 4e-6
        if t < best:
            best, bs = t, s
    bt = bs
    if mt_full and ntail:
        longs = math.ceil(float(nlong) * bs / 8.0)
        spare = int(math.ceil(longs / slots) * slots - longs)
        need, fit = int(math.ceil(tail_cost * bs)), spare * 8 // ntail
        bt = (fit if fit < 2 * bs else 2 * bs) if fit >= need else 2 * bs
        bt = 1 if bt < 1 else min(bt, smax)
    if o.get("tune_fc_slices", -1) > 0:
        bs = bt = min(o["tune_fc_slices"], chunks)
    if o.get("tune_fc_slices_tail", -1) > 0:
        bt = min(o["tune_fc_slices_tail"], chunks)
    return bs, (bt if ntail else 1), mt_full


def x3_plan(M, N, K, o):
    """-> (tile rows, slices, row tiles) of m3d_linear_bf16x3_forward.  A forced slice count above chunks / 8 + 1 with no forced tile height
    matches no candidate: the planner then leaves its empty initial plan (no row tiles: nothing would run) - a misuse of the tuning
    options that the table avoids by forcing the tile height as well."""
    chunks, nt = K // 32, cdiv(N, 128)
    force = o.get("tune_fc_slices", -1)
    best, best_t = (128, 1, 0), 1e30
    smax = min(chunks // 8 + 1, 64)
    for wr in (2, 4):
        tbm = 64 * wr
        tiles = cdiv(M, tbm) * nt
        slots = 64.0 if wr == 2 else 32.0
        rate = (1.65e14 if wr == 2 else 2.1e14) / (8.0 * slots)
        for s in range(1, smax + 1):
            if force > 0 and s != min(force, chunks):
                continue
            rounds = math.ceil(math.ceil(float(tiles) * s / 8.0) / slots)
            t = rounds * (2.0 * tbm * 128 * float(K) / s) / rate + rounds * 4e-6
            if s > 1:
                t += float(s) * M * N * 8.0 / 4e12 + 4e-6
            if t < best_t:
                best_t, best = t, (tbm, s, cdiv(M, tbm))
    w = o.get("tune_fc_x3_rows", -1)
    if w in (128, 256):
        s = best[1]
        if w != best[0]:
            s = int((512.0 if w == 128 else 256.0) / (cdiv(M, w) * nt))
            s = 1 if s < 1 else min(s, chunks // 8 + 1)
        if force > 0:
            s = min(force, chunks)
        best = (w, s, cdiv(M, w))
    return best


def x3b_slices(M, N, K, o):
    tiles, chunks = cdiv(M, 256) * cdiv(N, 256), K // 32
    if o.get("tune_fc_slices", -1) > 0:
        return min(o["tune_fc_slices"], chunks)
    return max(1, min(256 // tiles, chunks // 8 + 1, 64))


def plan(kind, M, N, K, o):
    """what m3d_linear_plan answers: dict(tile_rows, tile_cols, slices, slices_tail, full_row_tiles)"""
    if kind == 0:
        s, st, fm = make_plan(M, N, K, o)
        return dict(tile_rows=128, tile_cols=128, slices=s, slices_tail=st, full_row_tiles=fm)
    w = o.get("tune_fc_x3_rows", -1)
    if kind == 2 or (kind == 3 and w not in (128, 256) and (w == 512 or (M >= 384 and N >= 256))):
        s = x3b_slices(M, N, K, o)
        return dict(tile_rows=256, tile_cols=256, slices=s, slices_tail=s, full_row_tiles=cdiv(M, 256))
    tr, s, mt = x3_plan(M, N, K, o)
    return dict(tile_rows=tr, tile_cols=128, slices=s, slices_tail=s, full_row_tiles=mt)


def instance_of(kind, M, p):
    """the instance a plan names"""
    if kind == 0:
        rem = M - (cdiv(M, 128) - 1) * 128
        return "f32.full" if p["full_row_tiles"] == cdiv(M, 128) else ("f32.tail1" if rem <= 32 else "f32.tail2")
    if kind == 2:
        return "x3.w32"
    name = {(128, 128): "128", (256, 128): "256", (256, 256): "big"}[(p["tile_rows"], p["tile_cols"])]
    return ("x3." if kind == 1 else "f16.") + name


# ------------------------------------------------------------------ plans
def test_every_case_runs_the_instance_it_names(ops):
    from m3d import _lib
    assert len(set(T.CASES)) == len(T.CASES) and len({T.case_id(c) for c in T.CASES}) == len(T.CASES)
    for c in T.CASES:
        kind, o = T.kind_of(c), dict(c.knobs)
        assert set(o) <= {"tune_fc_slices", "tune_fc_slices_tail", "tune_fc_x3_rows"}
        mine = plan(kind, c.M, c.N, c.K, o)
        assert mine == T.expected_plan(c) and instance_of(kind, c.M, mine) == c.inst, (c, mine)
        if o:
            with _lib.tuning():
                for name, v in o.items():
                    _lib.set_option(name, v)
                assert ops.linear_plan(kind, c.M, c.N, c.K) == mine, (c, ops.linear_plan(kind, c.M, c.N, c.K))
            assert ops.linear_plan(kind, c.M, c.N, c.K) != mine, "%s needs no knob: the release library plans it" % (c,)
        else:
            assert ops.linear_plan(kind, c.M, c.N, c.K) == mine, (c, ops.linear_plan(kind, c.M, c.N, c.K))


def test_the_restated_planners_agree_with_the_library_over_a_grid(ops):
    """beyond the table: the restatement is the library's planner, release and under each knob"""
    from m3d import _lib
    shapes = [(M, N, K) for M in (1, 32, 33, 64, 65, 128, 129, 160, 161, 300, 384, 513, 1281) for N in (8, 72, 128, 255, 256, 1024)
              for K in (32, 64, 256, 800, 4096)] + [(40, 136, 87808), (1000, 1024, 87808), (1281, 1024, 87808)]
    for o in ({}, dict(tune_fc_slices=3), dict(tune_fc_x3_rows=128), dict(tune_fc_x3_rows=256), dict(tune_fc_x3_rows=512),
              dict(tune_fc_slices=2, tune_fc_slices_tail=5), dict(tune_fc_x3_rows=128, tune_fc_slices=70)):
        with _lib.tuning():
            for name, v in o.items():
                _lib.set_option(name, v)
            for kind in range(4):
                for s in shapes:
                    assert ops.linear_plan(kind, *s) == plan(kind, *s, o), (kind, s, o)
    assert ops.linear_plan(0, 64, 64, 30) is None and ops.linear_plan(1, 64, 64, 48) is None and ops.linear_plan(0, 64, 64, 36) is not None
    with pytest.raises(Exception):
        ops.linear_plan(4, 64, 64, 64)
    with pytest.raises(Exception):
        ops.linear_plan(0, 0, 64, 64)
    assert ops.lib().m3d_linear_plan(3, 64, 64, 64, None, None, None, None, None) == 0      # the outputs are optional


def test_the_query_is_the_workspace_and_the_launch_plan(ops):
    """the workspace sizes are the slice counts the query reports (one helper per kind behind all three)"""
    L = ops.lib()
    ws = (L.m3d_linear_workspace_bytes, L.m3d_linear_bf16x3_workspace_bytes, L.m3d_linear_bf16x3_w32_workspace_bytes,
          L.m3d_linear_f16x2_workspace_bytes)
    for c in T.CASES:
        if c.knobs:
            continue
        kind = T.kind_of(c)
        p = ops.linear_plan(kind, c.M, c.N, c.K)
        sm = max(p["slices"], p["slices_tail"])
        part = sm * c.M * c.N * 4 if sm > 1 else 0
        assert ws[kind](c.M, c.N, c.K) == (part + 256 if kind == 3 else max(part, 16)), c


# ------------------------------------------------------------------ coverage
def valid_rows(c):
    """rows in the last row tile"""
    tr = T.TILE[c.inst][0]
    return c.M - (cdiv(c.M, tr) - 1) * tr


def of(inst, cond=lambda c: True):
    return [c for c in T.CASES if c.inst == inst and cond(c)]


def own_slices(c):
    """the slice count and slice lengths of the path the instance names (the tail path for f32.tail*)"""
    return T.row_groups(c)[-1][2], T.slice_lengths(c)[-1]


@pytest.mark.parametrize("inst", T.INSTANCES)
def test_coverage_of_every_instance(inst):
    tr, tc = T.TILE[inst]
    tail = inst in ("f32.tail1", "f32.tail2")
    assert of(inst), inst
    assert all(c.M * c.N * c.K <= T.CAP_MAC for c in of(inst))
    assert of(inst, lambda c: cdiv(c.M, tr) >= 2 and cdiv(c.N, tc) >= 2)                          # two tiles along M and along N
    assert of(inst, lambda c: c.M % tr != 0 and cdiv(c.M, tr) >= 2)                               # a ragged last row tile
    assert of(inst, lambda c: c.N % tc != 0 and c.N % 32 != 0 and cdiv(c.N, tc) >= 2)             # a ragged last column tile
    if tail:                                                      # ragged in M by definition: the exact multiple is along N only
        assert of(inst, lambda c: c.N % tc == 0)
        assert of(inst, lambda c: c.M < 128) and of(inst, lambda c: c.M > 128 and c.slices != c.slices_tail)
        assert of(inst, lambda c: c.M > 128 and c.slices == 1 and c.slices_tail > 1) and of(inst, lambda c: c.slices > 1 and c.slices_tail == 1)
    else:
        assert of(inst, lambda c: c.M % tr == 0 and c.N % tc == 0)
    assert of(inst, lambda c: own_slices(c)[0] == 1) and of(inst, lambda c: own_slices(c)[0] > 1)
    assert of(inst, lambda c: len(set(own_slices(c)[1])) > 1)                                     # slices do not divide the chunks
    assert of(inst, lambda c: own_slices(c)[0] > 1 and 1 in own_slices(c)[1]) and of(inst, lambda c: own_slices(c)[0] > 1 and 2 in own_slices(c)[1])
    assert of(inst, lambda c: T.units(c)[-1] % 8 != 0)                                            # idle workgroups at the end of the unit map
    if inst not in ("x3.128", "f16.128"):                          # the release planners choose the 256-row tile at every size in reach
        assert of(inst, lambda c: not c.knobs), "no case of %s is planned by the release library" % inst
    if inst.startswith("f32"):
        assert all(c.K % 4 == 0 for c in of(inst))
    else:
        assert all(c.K % 32 == 0 and c.M > 32 for c in of(inst))


def test_coverage_across_the_table():
    rows = {valid_rows(c) % 32 for c in T.CASES} | {valid_rows(c) for c in T.CASES}
    assert {1, 31, 33} <= rows
    for inst in ("x3.128", "x3.256", "x3.w32", "f16.128", "f16.256", "f16.big"):
        got = {valid_rows(c) for c in of(inst)}
        assert {1, 31, 0} <= {v % 32 for v in got} and any(v > 32 and v % 32 == 1 for v in got), (inst, got)
    f32 = [c for c in T.CASES if c.inst.startswith("f32")]
    assert any(c.K == 32 for c in f32) and any(c.K % 32 != 0 for c in f32)
    assert any(c.K % 32 == 4 for c in f32)                                                        # a last chunk of one quad
    assert {valid_rows(c) for c in of("f32.tail1")} >= {1, 31, 32} and {valid_rows(c) for c in of("f32.tail2")} >= {33, 63, 64}
    assert any(c.K == 87808 and c.M <= 64 for c in T.CASES)
    # the thresholds of the f16x2 256 x 256 kernel, from both sides
    assert of("f16.big", lambda c: (c.M, c.N) == (384, 256) and not c.knobs) and of("f16.256", lambda c: (c.M, c.N) == (383, 256) and not c.knobs)
    assert of("f16.256", lambda c: c.M >= 384 and c.N < 256 and not c.knobs)
    # both reduce paths of the fp32 kernel across the m_full boundary: vector (N % 4 == 0) and scalar
    two = [c for c in f32 if len(T.row_groups(c)) == 2 and c.slices != c.slices_tail]
    assert any(c.N % 4 == 0 for c in two) and any(c.N % 4 != 0 for c in two)


# ------------------------------------------------------------------ exactness
@functools.lru_cache(maxsize=None)
def ints(c):
    x, w, b = T.integer_operands(c)
    for a in (x, w, b):
        a.setflags(write=False)
    return x, w, b


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_integer_case_is_exact(c):
    x, w, b = ints(c)
    fam = T.family(c)
    for a in (x, w, b):
        assert np.array_equal(a, np.rint(a))
    S = T.magnitude(x, w, b)
    assert float(S.max()) < 2.0 ** 24, float(S.max())
    y, yb = T.reference(x, w), T.reference(x, w, b, relu=True)
    assert (y > 0).any() and (y < 0).any() and (y + b[None, :] < 0).any() and b.any()              # the ReLU and the bias matter
    bounds = [None]
    if fam != "f32":
        chunks = c.K // 32
        bounds = [None, float(np.abs(x).max()), float(np.abs(x).max()) * 2.0 ** 8] if fam == "f16" else [None]
        for xb in bounds:
            px, pw = T.planes(c, x, xb), T.planes(c, w)
            assert np.array_equal(sum(px), x.astype(np.float64)) and np.array_equal(sum(pw), w.astype(np.float64))
            for ia, ib in T.DROPPED[fam]:                       # every dropped cross term is zero: no element pair has both planes
                assert not (np.abs(px[ia]) @ np.abs(pw[ib]).T).any()
            # every chunk of every row of x fills every plane; so does every chunk of every row of w, or (where an output cannot afford
            # that many probe products) of the columns the chunk is live for; every kept product is non-zero in every chunk
            for p in px:
                assert (np.abs(p).reshape(c.M, chunks, 32).sum(2) > 0).all()
            for p in pw:
                filled = np.abs(p).reshape(c.N, chunks, 32).sum(2) > 0
                assert filled.all() if T.live_period(c) == 1 else (filled.any(0).all() and c.N >= T.live_period(c))
            for ia, ib in T.PRODUCTS[fam]:
                assert ((np.abs(px[ia]).sum(0) > 0) & (np.abs(pw[ib]).sum(0) > 0)).reshape(chunks, 32).any(1).all(), (ia, ib)
        if fam == "f16":
            assert float(np.abs(x).max()) == float(np.abs(w).max()) == T.F16_TWO + 3
    for xb in bounds:
        assert T.cut_is_exact(c, x, w, xb)                        # the GPU test's condition for running a bound mode
        for bias, relu, ref in ((None, False, y), (b, True, yb)):
            got = T.emulate(c, x, w, bias, relu, np.float32, x_bound=xb)
            assert np.array_equal(got, T.expected_buffer(ref)), (T.case_id(c), xb, relu)


def test_cut_is_exact_tells_a_scale_that_is_not():
    """an x bound 2^30 above max |x| pushes the low plane of the two-plane probes below fp16's subnormals: the planes no longer sum to x,
    the emulation misses the reference, and cut_is_exact says so (the GPU test would not run that bound mode)"""
    c = next(c for c in T.CASES if c.inst == "f16.256")
    x, w, b = ints(c)
    xb = float(np.abs(x).max()) * 2.0 ** 30
    assert not T.cut_is_exact(c, x, w, xb)
    assert not np.array_equal(T.emulate(c, x, w, None, False, np.float32, x_bound=xb), T.expected_buffer(T.reference(x, w)))


# ------------------------------------------------------------------ defects
def caught(c, d):
    x, w, b = ints(c)
    ref = T.expected_buffer(T.reference(x, w, b, relu=True))
    got = T.emulate(c, x, w, b, True, np.float32, defect=d)
    plain = T.emulate(c, x, w, None, False, np.float32, defect=d)
    return not np.array_equal(got, ref) or not np.array_equal(plain, T.expected_buffer(T.reference(x, w)))


@pytest.mark.parametrize("d", T.DEFECTS)
def test_every_defect_is_caught(d):
    """by the GPU test's own comparison: the buffer (out and the sentinels around it) against the fp64 reference, bit for bit"""
    cases = [c for c in T.CASES if T.defect_applies(c, d) and c.K <= 4096]
    assert cases, d
    hits = [c for c in cases if caught(c, d)]
    assert hits, "no case catches %s" % d
    # every instance the defect can occur in catches it
    assert {c.inst for c in hits} == {c.inst for c in cases}, (d, {c.inst for c in cases} - {c.inst for c in hits})


def test_defects_apply_where_they_should():
    insts = lambda d: {c.inst for c in T.CASES if T.defect_applies(c, d)}
    every = set(T.INSTANCES)
    for d in ("short_slice", "bias_per_slice", "relu_per_slice", "row_mask_short", "row_mask_long", "col_mask_short", "col_mask_long",
              "col_block_neighbour"):
        assert insts(d) == every, (d, every - insts(d))
    assert insts("tail_full_slices") == {"f32.tail1", "f32.tail2"}
    assert insts("drop_low_product") == insts("dup_product") == {i for i in every if not i.startswith("f32")}


# ------------------------------------------------------------------ the bound
WORST = {}


@pytest.mark.parametrize("c", [c for c in T.CASES], ids=T.case_id)
def test_emulation_stays_inside_the_bound_on_random_data(c):
    x, w, b = T.random_operands(c)
    rows = np.abs(x).max(1)
    assert not w[c.N // 2].any() and (c.M < 64 or (not x[3].any() and rows.max() / rows[rows > 0].min() >= 2.0 ** 16))
    for bias, relu in ((None, False), (b, True)):
        y, E, S = T.bound(c, x, w, bias, relu)
        got = T.emulate(c, x, w, bias, relu, np.float32)[:c.M * c.N].reshape(c.M, c.N).astype(np.float64)
        assert np.isfinite(got).all()
        zero = S == 0                                               # nothing to sum: exactly the bias (or its ReLU)
        assert zero.any() and np.array_equal(got[zero], y[zero])
        ratio = float((np.abs(got - y) / np.maximum(E, 1e-300)).max())
        WORST[c.inst] = max(WORST.get(c.inst, 0.0), ratio)
        assert ratio <= 1.0, (T.case_id(c), relu, ratio)
    print("linear forward emulation: worst |got - y| / bound so far %s %.4f" % (c.inst, WORST[c.inst]))
