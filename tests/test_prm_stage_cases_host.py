"""CPU: the stage references of tests/prm_stage_cases.py ARE the reference's rule - chained seed -> prepare -> dgrad -> ... -> stem ->
scatter they reproduce oracle.prm_backward in fp64 - and the case table reaches every kernel the library's host queries name
(m3d_prm_prepare_plan, m3d_prm_stem_dgrad_plan, m3d_conv3d_direct_plan), holds the preconditions of the exact comparison, keeps an fp32
evaluation inside every bound, and its exact comparison catches the mutants a kernel could be."""
import ctypes as C

import numpy as np
import pytest
import torch

import prm_stage_cases as T

F32, F64 = T.F32, T.F64


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import LIB_PATH
    lib = C.CDLL(LIB_PATH)
    lib.m3d_prm_strip_geometry.restype = C.c_int64
    return lib


# ------------------------------------------------------------------ layouts
def test_strip_geometry_is_the_library_s(L):
    for n in range(1, 101):
        for P in (1, 3, 37):
            for mode in (1, 2):
                pitch, lead = C.c_int32(-1), C.c_int32(-1)
                Ls = L.m3d_prm_strip_geometry(n, mode, P, C.byref(pitch), C.byref(lead))
                assert T.strip_geometry(n, mode, P) == (pitch.value, lead.value, Ls), (n, mode, P)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n", [1, 5, 16, 18])
def test_layouts_round_trip(n, mode):
    rng = np.random.default_rng(n * 10 + mode)
    P, Cc = 3, 2
    win = rng.integers(1, 9, (P, Cc, n, n, n)).astype(F32)           # no zeros: a dropped voxel shows
    strip = T.pack_strip(win, mode)
    pitch, lead, Ls = T.strip_geometry(n, mode, P)
    assert strip.shape == (Cc, n, n, Ls)
    assert np.array_equal(T.unpack_strip(strip, mode, P, n), win)
    gaps = T.gap_columns(mode, P, n)
    assert len(gaps) == Ls - P * n and not strip[..., gaps].any() and np.count_nonzero(strip) == win.size
    assert np.isnan(T.pack_strip(win, mode, fill=np.nan)[..., gaps]).all()
    # slab strips: plane k of the slab = plane k - origin_z of the window; what falls outside the slab is dropped
    oz, zn = np.array([-2, 1, n + 3]), n + 1
    slab = T.pack_strip(win, mode, oz, zn)
    assert slab.shape == (Cc, zn, n, Ls)
    back = T.unpack_strip(slab, mode, P, n, oz)
    for p in range(P):
        kept = [i for i in range(n) if 0 <= i + oz[p] < zn]
        assert np.array_equal(back[p][:, kept], win[p][:, kept])
        for i in kept:
            assert np.array_equal(slab[:, i + oz[p], :, lead + p * pitch:lead + p * pitch + n], win[p][:, i])
        assert not back[p][:, [i for i in range(n) if i not in kept]].any()
    assert T.pack_strip(win, 0) is win


# ------------------------------------------------------------------ the table reaches every kernel
def prep_plan(L, c, P=3):
    return L.m3d_prm_prepare_plan(c.C, P, c.U, int(c.pool), c.border, c.out_l, int(c.out_slab), c.shape[0])


def test_every_prepare_kernel_is_reached_at_every_layout(L):
    seen = {}
    for c in T.PREP_CASES:
        rc = prep_plan(L, c)
        assert rc >= 0 and T.PREPARE_KERNELS[rc] == c.kernel, (c, rc)
        seen.setdefault(c.kernel, []).append(c)
    assert set(seen) == set(T.PREPARE_KERNELS)
    for kernel, cases in seen.items():
        outs = {"element": {0, 1}, "pool": {0, 1, 2}}.get(kernel, {2})
        assert {c.out_l for c in cases} == outs, kernel
        for out_l in outs:
            assert {c.in_l for c in cases if c.out_l == out_l} == {0, 1, 2}, (kernel, out_l)
        assert {c.in_slab for c in cases} == {False, True}, kernel
        assert {c.out_slab for c in cases} == {False, True}, kernel
        assert {c.up_off for c in cases} == {False, True} and {c.scale for c in cases} == {False, True}, kernel
        assert {c.origins for c in cases} == {"edge", "out"}, kernel
        assert any(c.in_slab and c.shape[0] // (2 if c.pool else 1) < c.U for c in cases)
    assert {(c.U, c.border) for c in seen["element"]} == {(U, b) for U in (1, 3, 5) for b in (1, 2)}
    assert {c.U + 2 * c.border for c in seen["quad<8>"]} >= {16, 18}
    assert {c.U + 2 * c.border for c in seen["quad<16>"]} == {38, 40}
    assert all(c.U + 2 * c.border >= 62 and c.C <= 2 for c in seen["quad<32>"])
    assert {(c.U, c.border) for c in seen["pool"]} == {(U, b) for U in (3, 7) for b in (1, 2)}
    assert all(s % 2 == 1 for c in seen["pool"] for s in c.shape)     # MaxPool3d's floor applies
    for c in T.PREP_CASES:                                              # a wholly outside window exists where the table says so
        o = T.origins_for(c.origins, tuple(s // 2 for s in c.shape) if c.pool else c.shape, c.U)
        up = tuple(s // 2 for s in c.shape) if c.pool else c.shape
        outside = [T.inside_box(q, c.U, up) is None for q in o]
        assert outside == [False, c.origins == "out", False], c
        mul = 2 if c.pool else 1                                       # the OUTPUT windows stick out of the map at both ends
        hi = mul * o[2] - c.border + mul * c.U + 2 * c.border
        assert (mul * o[0] - c.border < 0).all() and hi[0] > c.shape[0] and hi[2] > c.shape[2]


def test_prepare_plan_is_the_launcher_s_rule(L):
    EINVAL, EUNSUPPORTED = -1, -4
    assert L.m3d_prm_prepare_plan(3, 3, 5, 0, 1, 0, 0, 1) == 0
    assert L.m3d_prm_prepare_plan(3, 0, 5, 0, 1, 0, 0, 1) == 0          # no peaks: the id the shape would run
    assert L.m3d_prm_prepare_plan(3, 3, 5, 0, 1, 0, 1, 8) == EINVAL     # slab without strip
    assert L.m3d_prm_prepare_plan(3, 3, 5, 0, 1, 3, 0, 8) == EINVAL
    assert L.m3d_prm_prepare_plan(0, 3, 5, 0, 1, 0, 0, 8) == EINVAL
    assert L.m3d_prm_prepare_plan(3, 3, 5, 0, 1, 0, 0, 0) == EINVAL
    assert L.m3d_prm_prepare_plan(3, 3, 99, 0, 1, 0, 0, 8) == EUNSUPPORTED      # Wn 101
    assert L.m3d_prm_prepare_plan(3, 3, 98, 0, 1, 0, 0, 8) == 0
    assert L.m3d_prm_prepare_plan(3, 3, 5, 1, 3, 0, 0, 8) == EUNSUPPORTED       # pool: the shell covers borders <= 2
    assert L.m3d_prm_prepare_plan(3, 3, 99, 1, 1, 0, 0, 8) == EUNSUPPORTED
    assert L.m3d_prm_prepare_plan(3, 3, 98, 1, 1, 2, 0, 8) == 4
    assert L.m3d_prm_prepare_plan(70000, 3, 5, 0, 1, 0, 0, 8) == EUNSUPPORTED
    anchors = {5: 1, 16: 1, 18: 1, 38: 2, 40: 2, 62: 3, 64: 3, 100: 3}
    for Wn in range(3, 101):
        pitch, lead, Ls = T.strip_geometry(Wn, 2, 3)
        nq = Ls // 4 - 2 * (pitch // 4)                                 # quads of the last cell with the strip's tail
        want = 1 if nq <= 8 else 2 if nq <= 16 else 3
        assert anchors.get(Wn, want) == want, (Wn, nq)
        assert L.m3d_prm_prepare_plan(3, 3, Wn - 2, 0, 1, 2, 0, 8) == want, Wn
        assert L.m3d_prm_prepare_plan(3, 3, Wn - 2, 0, 1, 1, 0, 8) == 0


def test_every_stem_layout_is_reached(L):
    assert L.m3d_prm_stem_dgrad_plan(0) == -1
    assert (L.m3d_prm_stem_dgrad_plan(84), L.m3d_prm_stem_dgrad_plan(40)) == (0, 1)     # the two nets' windows
    for c in T.STEM_CASES:
        assert T.STEM_LAYOUTS[L.m3d_prm_stem_dgrad_plan(c.win)] == c.layout, c
    for layout in T.STEM_LAYOUTS:
        assert {c.C for c in T.STEM_CASES if c.layout == layout} >= {3, 32}
    assert any(c.win ** 3 % 4 for c in T.STEM_CASES) and any(c.win ** 3 % 4 == 0 for c in T.STEM_CASES)     # both per-peak sum paths
    assert {c.U for c in T.FUSED_CASES} == {18, 40}
    for U in (18, 40):
        cs = [c for c in T.FUSED_CASES if c.U == U]
        assert {c.in_l for c in cs} == {0, 1, 2} and {c.slab for c in cs} == {False, True} and {c.up_off for c in cs} == {False, True}
        assert L.m3d_prm_stem_dgrad_fused_supported(32, U) == 1
    assert all(c.P == 2 and c.pooled[0] <= 6 for c in T.FUSED_CASES if c.U == 40)


def test_windowed_cases_reach_three_direct_conv_variants(L):
    ids = set()
    for c in T.WINDOWED_CASES:
        v = C.c_int(-1)
        assert L.m3d_conv3d_direct_plan(c.P, c.cg, c.cx, c.win, c.win, c.win, 3, 0, C.byref(v), None, None, None, None, None, None) == 0
        assert v.value == c.variant, (c, v.value)
        assert c.cg % 2 == 1 and c.cx % 32 != 0
        ids.add(v.value)
    assert len(ids) >= 3 and {c.win for c in T.WINDOWED_CASES} == {3, 7, 9, 18}
    assert {(c.win, c.P) for c in T.SMALL_CASES} == {(w, P) for w in (3, 5, 7) for P in (1, 37)}


# ------------------------------------------------------------------ exactness preconditions and the fp32 evaluation
def is_exact_fp32(a):
    return np.array_equal(a.astype(F32).astype(F64), a, equal_nan=True)


@pytest.mark.parametrize("c", T.PREP_CASES, ids=T.prep_id)
def test_prepare_exact_precondition_and_fp32_evaluation(c):
    inp = T.prep_inputs(c, True)
    for step in ("gup", "xnext", "norm"):
        assert is_exact_fp32(inp[step].astype(F64))
    n = inp["norm"]
    live = ~(n < T.EPS)
    assert np.array_equal((np.abs(n) + T.EPS)[live], np.abs(n)[live]) and np.all(np.log2(n[live]) % 1 == 0) and n[live].min() >= 2.0 ** -9
    assert 3 * 5 * 3 * 2 ** 9 < T.LIMIT                              # |gup| |xnext - off| |scale| / min norm
    y, o = T.prep_reference(c, inp)
    assert is_exact_fp32(y) and np.abs(y).max() < T.LIMIT
    y32, o32 = T.prep_reference(c, inp, dt=F32)
    T.same_bits(y32, y, "fp32 evaluation of the exact case")
    assert np.array_equal(o, o32)
    if c.origins == "out":
        assert not y[1].any()
    assert y[0].any() and y[2].any(), "a peak whose window is all zero checks nothing"

    inp = T.prep_inputs(c, False)
    y, _ = T.prep_reference(c, inp)
    y32, _ = T.prep_reference(c, inp, dt=F32)
    assert np.count_nonzero(y) > 0.2 * np.count_nonzero(T.prep_reference(c, dict(inp, norm=np.ones_like(inp["norm"])))[0])
    r = T.ratio(y32, y, T.bound_pointwise(y, T.k_prepare(c.up_off, c.scale)), T.prep_id(c))
    assert r <= 1.0, r


def test_cut_edges_are_in_the_data():
    for c in T.PREP_CASES[:6]:
        for exact in (True, False):
            inp = T.prep_inputs(c, exact)
            n, x = inp["norm"], inp["xnext"]
            assert (n == 0).any() and (n < 0).any() and ((n > 0) & (n < T.EPS)).any()
            assert (x == 0).any() and np.signbit(x[x == 0]).any() and (x == np.finfo(F32).tiny).any() and (x < 0).any()
            if not exact:
                for v in (T.EPS, np.nextafter(T.EPS, F32(0)), np.nextafter(T.EPS, F32(1)), F32(-1), F32(1e3), F32(1e-9)):
                    assert (n == v).any(), v


@pytest.mark.parametrize("c", T.SEED_CASES, ids=str)
def test_seed_reference(c):
    e = T.seed_inputs(c, True)
    y, o = T.ref_seed(e["peaks"], e["prob"], e["ncls"], e["wcls"], e["h"], e["off"])
    assert is_exact_fp32(y) and np.abs(y).max() < T.LIMIT and y.any()
    T.same_bits(T.ref_seed(e["peaks"], e["prob"], e["ncls"], e["wcls"], e["h"], e["off"], dt=F32)[0], y, "seed fp32")
    assert np.array_equal(o, e["peaks"][:, 1:])
    e = T.seed_inputs(c, False)
    y, _ = T.ref_seed(e["peaks"], e["prob"], e["ncls"], e["wcls"], e["h"], e["off"])
    y32, _ = T.ref_seed(e["peaks"], e["prob"], e["ncls"], e["wcls"], e["h"], e["off"], dt=F32)
    assert T.ratio(y32, y, T.bound_pointwise(y, 9), "seed") <= 1.0


@pytest.mark.parametrize("case", T.DEN_CASES, ids=str)
def test_den_pool_reference(case):
    for exact in (True, False):
        e = T.den_inputs(case, exact)
        y = T.ref_den_pool(e["argmax"], e["xnext"], e["norm"])
        y32 = T.ref_den_pool(e["argmax"], e["xnext"], e["norm"], dt=F32)
        if exact:
            T.same_bits(y32, y, "den fp32")
        assert T.ratio(y32, y, T.bound_pointwise(y, 1), "den") <= 1.0
        assert not (y < 0).any() and (y.size < 8 or ((y == 0).any() and (y > 0).any()))
        # the definition, voxel by voxel
        Cc, UD, UH, UW = e["argmax"].shape
        for idx in np.ndindex(Cc, UD, UH, UW):
            a = int(e["argmax"][idx])
            q = (idx[0], 2 * idx[1] + (a >> 2), 2 * idx[2] + ((a >> 1) & 1), 2 * idx[3] + (a & 1))
            n = e["norm"][q]
            want = F64(abs(n) + T.EPS) if (e["xnext"][idx] > 0 and not n < T.EPS) else 0.0
            assert y[idx] == want


@pytest.mark.parametrize("c", T.SCATTER_CASES, ids=str)
def test_scatter_reference(c):
    for exact in (True, False):
        e = T.scatter_inputs(c, exact)
        y = T.ref_scatter(e["win"], e["sums"], e["origin"], c.shape)
        y32 = T.ref_scatter(e["win"], e["sums"], e["origin"], c.shape, dt=F32)
        assert np.isnan(y[3]).all() and not np.isnan(y[:3]).any()
        if exact:
            T.same_bits(y32, y, "scatter fp32")
        assert T.ratio(y32, y, T.bound_pointwise(y, T.DIV), "scatter") <= 1.0
    assert [int(np.prod(c.shape)) % 4 for c in T.SCATTER_CASES] == [2, 0, 3]


@pytest.mark.parametrize("c", T.WINDOWED_CASES + T.SMALL_CASES, ids=T.dgrad_id)
def test_dgrad_reference(c):
    e = T.dgrad_inputs(c, True)
    y, ca = T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], want_cabs=True)
    assert ca.max() < T.LIMIT and is_exact_fp32(y) and y.any()
    T.same_bits(T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], dt=F32), y, "dgrad fp32", sums=True)
    assert ((e["full"] - e["off"]) < 0).any() and (e["w"] < 0).any()
    e = T.dgrad_inputs(c, False)
    y, ca = T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], want_cabs=True)
    y32 = T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], dt=F32)
    assert T.ratio(y32, y, T.bound_sum(y, ca, 27 * c.cg), T.dgrad_id(c), signs=False) <= 1.0


@pytest.mark.parametrize("c", T.STEM_CASES, ids=str)
def test_stem_reference(c):
    e = T.stem_inputs(c, True)
    y, s, ca = T.ref_stem(e["gn"], e["w"], e["data"], e["off"], e["origin"], want_cabs=True)
    assert ca.max() < T.LIMIT and s.max() < T.LIMIT and is_exact_fp32(y) and y.any() and (y == 0).any()
    y32, s32 = T.ref_stem(e["gn"], e["w"], e["data"], e["off"], e["origin"], dt=F32)
    T.same_bits(y32, y, "stem fp32", sums=True)
    T.same_bits(s32, s, "stem sums fp32")
    e = T.stem_inputs(c, False)
    y, s, ca = T.ref_stem(e["gn"], e["w"], e["data"], e["off"], e["origin"], want_cabs=True)
    y32, s32 = T.ref_stem(e["gn"], e["w"], e["data"], e["off"], e["origin"], dt=F32)
    b = T.bound_sum(y, ca, 125 * c.C, clamped=True)
    assert T.ratio(y32, y, b, str(c), signs=False) <= 1.0
    assert T.ratio_sums(s32, y32, y, b, c.win ** 3, str(c)) <= 1.0


@pytest.mark.parametrize("c", T.FUSED_CASES, ids=T.fused_id)
def test_fused_stem_exact_precondition(c):
    inp, y, s, o, ca = T.fused_reference(c, True)
    assert ca.max() < T.LIMIT and s.max() < T.LIMIT and is_exact_fp32(y) and set(np.unique(inp["den"])) == {0.0, 1.0}
    assert all(y[p].any() for p in range(c.P)) and np.array_equal(o, 2 * inp["origin_up"] - 2)
    if c.U == 18:                                                       # the fp32 evaluation (U = 40: the GPU test's cases only)
        inp, y, s, o, ca = T.fused_reference(c, False)
        y32, s32, _ = T.ref_stem_fused(inp["gup"], inp["origin_up"], inp["den"], inp["argmax"], inp["scale"], inp["w"], inp["data"], inp["off"],
                                       inp["xnext"], inp["up_off"], dt=F32)
        b = T.bound_sum(y, ca, 125 * 32, T.k_fused(c.up_off, c.scale), clamped=True)
        assert T.ratio(y32, y, b, T.fused_id(c), signs=False) <= 1.0
        assert T.ratio_sums(s32, y32, y, b, (2 * c.U + 4) ** 3, T.fused_id(c)) <= 1.0


def test_fused_stem_is_prepare_then_stem():
    """the fused reference (den map) against the two-stage one (prepare with pool and border 2, then the stem), on exact data"""
    c = T.FUSED_CASES[1]
    inp, y, s, o, _ = T.fused_reference(c, True)
    rng = np.random.default_rng(5)
    norm = T.exact_norm((32,) + inp["data"].shape, rng)
    xnext = inp["xnext"]
    den = T.ref_den_pool(inp["argmax"], xnext, norm).astype(F32)
    live = den > 0
    assert np.array_equal(den[live], T.pooled(np.abs(norm), inp["argmax"])[0][live])
    y1, s1, o1 = T.ref_stem_fused(inp["gup"], inp["origin_up"], den, inp["argmax"], inp["scale"], inp["w"], inp["data"], inp["off"],
                                  xnext, inp["up_off"])
    gn, o2 = T.ref_prepare(inp["gup"], inp["origin_up"], True, 2, inp["argmax"], xnext, inp["scale"], norm, inp["up_off"])
    y2, s2 = T.ref_stem(gn, inp["w"], inp["data"], inp["off"], o2)
    assert np.array_equal(o1, o2) and np.array_equal(y1, y2) and np.array_equal(s1, s2) and y1.any()


# ------------------------------------------------------------------ mutants: the exact comparison catches each
def first(pred):
    return next(c for c in T.PREP_CASES if pred(c))


def test_mutants_are_caught():
    c = first(lambda c: c.kernel == "pool" and c.out_l == 1 and c.scale)
    inp = T.prep_inputs(c, True)
    y, o = T.prep_reference(c, inp)
    T.same_bits(y.astype(F32), y, "itself")

    with pytest.raises(AssertionError):                                 # the |n| < eps cut in place of n < eps
        T.same_bits(T.prep_reference(c, inp, abs_cut=True)[0], y, "abs cut")
    swapped = ((inp["argmax"] & 2) | ((inp["argmax"] & 1) << 2) | (inp["argmax"] >> 2)).astype(np.uint8)
    with pytest.raises(AssertionError):                                 # arg-max child bit order swapped
        T.same_bits(T.prep_reference(c, dict(inp, argmax=swapped))[0], y, "child bits")
    for axis in range(3):                                               # an origin off by one
        shifted = inp["origin_up"].copy()
        shifted[:, axis] += 1
        ym, om = T.prep_reference(c, dict(inp, origin_up=shifted))
        assert not np.array_equal(om, o)
        with pytest.raises(AssertionError):
            T.same_bits(ym, y, "origin")
    # a separator column left unwritten: the output is pre-filled with NaN and every column of the strip is compared
    want = T.prep_layouts(c, inp, y, o)[1]
    for col in T.gap_columns(c.out_l, 3, y.shape[2]):
        got = want.astype(F32)
        got[:, 1, 2, col] = np.nan
        with pytest.raises(AssertionError):
            T.same_bits(got, want, "separator")
    # the same in the non-pool kernel's rule
    c = first(lambda c: c.kernel == "element" and c.U == 3)
    inp = T.prep_inputs(c, True)
    with pytest.raises(AssertionError):
        T.same_bits(T.prep_reference(c, inp, abs_cut=True)[0], T.prep_reference(c, inp)[0], "abs cut")

    # one tap dropped: windowed conv, small GEMM and the stem
    for c, (inputs, run) in [(T.WINDOWED_CASES[0], (T.dgrad_inputs, lambda e: T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"]))),
                             (T.SMALL_CASES[-1], (T.dgrad_inputs, lambda e: T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"]))),
                             (T.STEM_CASES[2], (T.stem_inputs, lambda e: T.ref_stem(e["gn"], e["w"], e["data"], e["off"], e["origin"])[0]))]:
        e = inputs(c, True)
        y = run(e)
        taps = np.argwhere(e["w"] > 0)
        for t in (taps[0], taps[len(taps) // 2], taps[-1]):
            w = e["w"].copy()
            w[tuple(t)] = 0
            with pytest.raises(AssertionError):
                T.same_bits(run(dict(e, w=w)), y, "tap", sums=True)


# ------------------------------------------------------------------ composition: the chained references are oracle.prm_backward
def layers_of(saved):
    layers, prob = [], None
    for rec in saved:
        k = rec["kind"]
        if k == "conv":
            layers.append(dict(name=rec["name"], xo=rec["xo"][0].numpy(), norm=rec["norm"][0].numpy(), pad=rec["pad"], scale=None, mask=None,
                               idx=None))
        elif k == "bn":
            layers[-1]["scale"] = rec["scale"].numpy()
        elif k == "relu":
            layers[-1]["mask"] = rec["mask"][0].numpy()
        elif k == "pool":
            layers[-1]["idx"] = rec["idx"][0].numpy()
        elif k == "sigmoid":
            prob = rec["y"][0].numpy()
    return layers, prob


def chain(P, layers, prob, peak):
    """seed -> (prepare -> dgrad) per layer, top down -> prepare -> stem -> scatter, for one peak (a, s, h, w)"""
    top = layers[-1]
    wcls = P[top["name"] + ".weight"].numpy()
    g, origin = T.ref_seed(np.array([peak], np.int32), prob, top["norm"], wcls.reshape(wcls.shape[0], -1), top["xo"], 0.0)
    g = g.reshape(1, -1, 1, 1, 1)
    for Lr in reversed(layers[:-1]):
        mask = Lr["mask"]
        pool = Lr["idx"] is not None
        argmax, xnext = None, mask.astype(F64)
        if pool:
            D, H, W = mask.shape[1:]
            idx = Lr["idx"]
            z, y, x = idx // (H * W), (idx // W) % H, idx % W
            argmax = ((z % 2) * 4 + (y % 2) * 2 + (x % 2)).astype(np.uint8)
            xnext = np.take_along_axis(mask.reshape(mask.shape[0], -1), idx.reshape(idx.shape[0], -1), 1).reshape(idx.shape).astype(F64)
        gn, origin = T.ref_prepare(g, origin, pool, Lr["pad"], argmax, xnext, Lr["scale"], Lr["norm"])
        w = P[Lr["name"] + ".weight"].numpy()
        if Lr["pad"] == 2:
            y, s = T.ref_stem(gn, w, Lr["xo"][0], 0.0, origin, boxed=True)
            return T.ref_scatter(y, s, origin, Lr["xo"].shape[1:])[0], y.shape[1]
        g = T.ref_dgrad(gn, w, Lr["xo"], 0.0, origin)


@pytest.mark.parametrize("stride,shape,peaks", [
    (4, (12, 12, 12), [(0, 0, 0, 0), (2, 1, 1, 1), (1, 2, 2, 2), (0, 2, 0, 1)]),     # feature map 3^3: corners and the interior
    (8, (8, 16, 24), [(1, 0, 1, 2), (0, 0, 0, 1)]),
], ids=["stride4", "stride8"])
def test_chained_references_are_the_oracle_s_backward(stride, shape, peaks):
    import oracle as O
    P = O.make_params(stride=stride, num_anchors=3, head=False, seed=stride, dtype=torch.float64)
    data = torch.randn((1, 1) + shape, generator=torch.Generator().manual_seed(stride), dtype=torch.float64)
    with torch.no_grad():
        feat, prob, deltas, saved = O.prm_forward(P, O.Cfg(stride=stride), data)
        layers, pr = layers_of(saved)
        assert tuple(prob.shape[2:]) == tuple(s // stride for s in shape)
        for peak in peaks:
            want = O.prm_backward(P, saved, (0,) + peak, prob.shape)[0].numpy()
            got, win = chain(P, layers, pr, peak)
            assert win == (84 if stride == 8 else 40)
            assert want.max() > 0 and np.isfinite(want).all()
            assert np.abs(got - want).max() <= 1e-12 * want.max(), (peak, np.abs(got - want).max(), want.max())
