"""CPU: the tables of tests/prm_small_cases.py reach what they claim (computed from the constants mirrored from csrc/prm_small_f16.hip and
csrc/prm_small.hip), their exact operands are exact, the NumPy emulation of the unmutated launch equals the fp64 reference bit for bit
and fits every bound (so the reference side is known to fit before anything runs on a GPU), the exact comparison catches every seeded
defect on every case the defect applies to, and the library's support query agrees with the tables."""
import ctypes as C

import numpy as np
import pytest
import torch

import f16x2_contract as K
import prm_small_cases as S
import prm_stage_cases as T

F32, F64 = np.float32, np.float64
KINDS = ("f16", "f32")
ALL_CASES = [(k, c) for k in KINDS for c in S.CASES[k]]
ALL_PROBES = [(win, which) for win in (3, 5, 7) for which in S.PROBES]


def kid(v):
    return v if isinstance(v, str) else S.case_id(v) if isinstance(v, S.SmallCase) else str(v)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import LIB_PATH
    lib = C.CDLL(LIB_PATH)
    for f in ("m3d_prm_small_dgrad_packed_bytes", "m3d_prm_small_dgrad_f16_packed_bytes", "m3d_prm_small_dgrad_f16_workspace_bytes"):
        getattr(lib, f).restype = C.c_size_t
    return lib


# ------------------------------------------------------------------ the tables reach what they claim
def test_mirrored_constants():
    assert [S.geom("f16", w)[3:] for w in (3, 5, 7)] == [(5, 125, 128, 6, 16), (7, 343, 256, 4, 16), (9, 729, 256, 2, 16)]
    assert [S.geom("f32", w)[3:] for w in (3, 5, 7)] == [(5, 125, 128, 6, 4), (7, 343, 128, 3, 4), (9, 729, 128, 2, 4)]
    assert all(c.cg % 16 == 0 for c in S.F16_CASES + tuple(S.PROBE_SHAPES.values()) + (S.CLAMP_CASE,))
    assert len(set(S.F16_CASES)) == 8 and len(set(S.F32_CASES)) == 6


def test_the_rows_reach_what_the_table_says():
    """the claims written next to the rows of F16_CASES / F32_CASES, from the geometry"""
    wg = lambda kind, c: S.workgroups(kind, S.SmallCase(*c))
    w = wg("f16", (3, 16, 24, 1))
    assert w == [(0, 0, 27, 1, 5)] and S.nchunk("f16", S.SmallCase(3, 16, 24, 1)) == 1
    w = wg("f16", (3, 48, 33, 24))                                      # 648 columns: 5 workgroups + 8 columns
    assert len(w) == 6 and w[4][:4] == (512, 18, 128, 6) and 512 - 18 * 27 == 26 and w[5][2:] == (8, 1, 5)
    w = wg("f16", (3, 256, 64, 19))
    assert 19 * 27 == 4 * 128 + 1 and len(w) == 5 and w[4][2] == 1 and S.nchunk("f16", S.SmallCase(3, 256, 64, 19)) == 16
    w = wg("f16", (5, 32, 40, 44))
    assert w[20][:4] == (5120, 40, 256, 4) and 5120 - 40 * 125 == 120
    assert S.nchunk("f16", S.SmallCase(5, 80, 96, 3)) == 5
    w = wg("f16", (7, 16, 32, 1))
    assert [x[2] for x in w] == [256, 87]
    assert any(x[3] == 2 for x in wg("f16", (7, 64, 33, 4))) and S.nchunk("f16", S.SmallCase(7, 64, 33, 4)) == 4
    assert S.nchunk("f16", S.SmallCase(7, 256, 24, 2)) == 16
    assert any(x[3] == 6 for x in wg("f32", (3, 64, 33, 24))) and S.nchunk("f32", S.SmallCase(3, 64, 33, 24)) == 16
    w = wg("f32", (3, 12, 40, 128))
    assert len(w) == 27 and all(x[2] == 128 for x in w)
    assert wg("f32", (5, 8, 40, 44))[41][3] == 3
    assert S.nchunk("f32", S.SmallCase(5, 130, 24, 3)) == 33 and 130 % 4 == 2
    assert S.nchunk("f32", S.SmallCase(7, 256, 64, 2)) == 64


@pytest.mark.parametrize("kind", KINDS)
def test_structural_conditions(kind):
    for win in (3, 5, 7):
        g = S.geom(kind, win)
        wgs = [w for c in S.CASES[kind] if c.win == win for w in S.workgroups(kind, c)]
        assert any(used == g.PK for _, _, _, used, _ in wgs), (win, "all slots")
        assert any(beyond > 0 for _, _, _, _, beyond in wgs), (win, "slots beyond P")
        assert any(ncol < g.cols for _, _, ncol, _, _ in wgs), (win, "partial workgroup")
        assert any(n0 % g.V and used >= 2 for n0, _, _, used, _ in wgs), (win, "a workgroup that starts mid-peak and spans peaks")
    if kind == "f32":
        assert any((c.P * c.win ** 3) % 128 == 0 for c in S.F32_CASES), "a whole number of workgroups"
    nch = {S.nchunk(kind, c) for c in S.CASES[kind]}
    if kind == "f16":
        assert 1 in nch and 16 in nch and any(n % 2 and n >= 3 for n in nch) and any(n % 2 == 0 and n >= 4 for n in nch)
    else:
        assert 1 in nch and any(n >= 16 for n in nch) and any(c.cg % 4 for c in S.F32_CASES if c.cg > 4)
    cxs = {c.cx for c in S.CASES[kind]}
    assert any(x < 32 for x in cxs) and 33 in cxs and any(x % 32 == 0 for x in cxs) and any(x > 32 and x % 32 for x in cxs)
    both = {c.cx for k in KINDS for c in S.CASES[k]}                    # the two kernels share the epilogue's channel rule
    assert any(x < 32 for x in both) and 32 in both and 33 in both and any((x + 31) // 32 >= 3 for x in both)
    # the families: every one on three f16 cases, benign / heavy / zero on three fp32 cases, one per window size
    table = S.bounded_table(kind)
    fams = S.FAMILIES if kind == "f16" else S.F32_FAMILIES
    for f in fams:
        assert {c.win for c, ff in table if ff == f} == {3, 5, 7}
    assert {c for c, f in table if f == "benign"} == set(S.CASES[kind]) and len(S.FAMILIES) == 9


@pytest.mark.parametrize("kind,c", ALL_CASES, ids=kid)
def test_origins(kind, c):
    e = S.exact_inputs(kind, c)
    o = e["origin"]
    assert tuple(o[0]) == (-1, -2, -1)
    if c.P >= 3:
        assert T.inside_box(o[2], c.win, S.map_shape(c)) is None
    m, inmap = S.multiplier(e)
    assert inmap.any() and not inmap.all() and (m < 0).any() and (e["w"] < 0).any()


def test_support_query_agrees_with_the_tables(L):
    for c in S.F16_CASES + tuple(S.PROBE_SHAPES.values()) + (S.CLAMP_CASE,):
        assert L.m3d_prm_small_dgrad_f16_supported(c.cg, c.cx) == 1, c
        nch, ncb = c.cg // 16, (c.cx + 31) // 32
        assert L.m3d_prm_small_dgrad_f16_packed_bytes(c.cg, c.cx) == ncb * nch * 27 * 2 * 64 * 16 + 256
    for c in S.F32_CASES:
        assert L.m3d_prm_small_dgrad_f16_supported(c.cg, c.cx) == (1 if c.cg % 16 == 0 else 0), c
        assert L.m3d_prm_small_dgrad_packed_bytes(c.cg, c.cx) == ((c.cx + 31) // 32) * S.nchunk("f32", c) * 2 * 7 * 64 * 4 * 4
    assert any(L.m3d_prm_small_dgrad_f16_supported(c.cg, c.cx) == 0 for c in S.F32_CASES)
    assert L.m3d_prm_small_dgrad_f16_supported(0, 8) == 0 and L.m3d_prm_small_dgrad_f16_packed_bytes(7, 40) == 0
    assert L.m3d_prm_small_dgrad_f16_workspace_bytes(S.F16_MAX_PEAKS) == 4 * S.F16_MAX_PEAKS + 256


# ------------------------------------------------------------------ exact operands: preconditions, and the emulation equals the reference
def is_exact_fp32(a):
    return np.array_equal(a.astype(F32).astype(F64), a)


@pytest.mark.parametrize("kind,c", ALL_CASES, ids=kid)
def test_exact_case(kind, c):
    e, y, ca = S.exact_reference(kind, c)
    unit = (2.0 ** e["kp"]).reshape(-1, 1, 1, 1, 1)
    assert (ca / unit).max() < S.LIMIT and is_exact_fp32(y)
    assert y[0].any() and 2 * sum(bool(y[p].any()) for p in range(c.P)) >= c.P     # the seeded origins put some windows outside
    if kind == "f16":
        assert e["kp"].min() >= -20 and e["kp"].max() <= 20 and (c.P == 1 or (e["kp"].min(), e["kp"].max()) == (-20, 20))
        assert np.array_equal(np.abs(e["gn"]).reshape(c.P, -1).max(1), 3 * 2.0 ** e["kp"])
    T.same_bits(T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], dt=F32), y, "fp32 evaluation", sums=True)
    T.same_bits(S.emulate_case(kind, e), y, "emulation of " + S.case_id(c), sums=True)


def pieces(e):
    """the cut pieces of both operands (unscaled fp64): (gh, gl, wh, wl)"""
    gn, wr = torch.from_numpy(e["gn"]), torch.relu(torch.from_numpy(e["w"]))
    gh, gl = K.cut(gn, gn.abs().amax(dim=(1, 2, 3, 4), keepdim=True))
    wh, wl = K.cut(wr, float(wr.max()))
    return gh, gl, wh, wl


@pytest.mark.parametrize("win,which", ALL_PROBES, ids=kid)
def test_probe(win, which):
    c = S.PROBE_SHAPES[win]
    e, y, ca = S.probe_reference(win, which)
    gh, gl, wh, wl = pieces(e)
    # the cut loses nothing: h + l is the operand, and the dropped l l product vanishes everywhere
    assert torch.equal(gh + gl, torch.from_numpy(e["gn"]).double()) and torch.equal(wh + wl, torch.relu(torch.from_numpy(e["w"])).double())
    assert not K.dgrad_op(gl.abs(), wl.abs()).any()
    assert (gl if which == "gn" else wl).any(), "the probe does not fill a lo piece"
    assert not (wl if which == "gn" else gl).any()
    # every partial sum of the pieces' products is exact: their magnitudes add to less than 2^24 in the peak's own units
    unit = torch.from_numpy(2.0 ** e["kp"]).view(-1, 1, 1, 1, 1)
    cp = K.dgrad_op(gh.abs() + gl.abs(), wh.abs() + wl.abs()) / unit
    assert float(cp.max()) < S.LIMIT
    m, inmap = S.multiplier(e)
    assert is_exact_fp32(y) and y.any()
    if which == "gn":
        n = K.terms(K.dgrad_op, torch.from_numpy(e["gn"]), torch.relu(torch.from_numpy(e["w"])))[3]
        assert float(n.max()) == 1.0                                    # every output is one product
        chans, vox = S.probe_positions(c)
        assert {ch % 16 // 8 for ch in chans} == {0, 1} and {ch // 16 % 2 for ch in chans} == {0, 1} and {ch // 16 for ch in chans} == {0, 1, 2}
        assert {0, c.win ** 3 // 2, c.win ** 3 - 1} <= set(vox)         # the centre voxel meets all 27 taps, the corners the first / last
        assert all(np.count_nonzero(e["gn"][p]) == 1 for p in range(c.P))
    else:
        assert set(np.unique(np.abs(m[inmap]))) <= {0.0, 1.0, 2.0, 4.0}
        ci, co, tz, ty, tx = S.PROBE_W_AT[win]
        big = e["w"][ci, co, tz, ty, tx]
        assert 2 ** 21 <= big < 2 ** 22 and big % 2 == 1 and np.count_nonzero(np.abs(e["w"]) > 2) == 1
    T.same_bits(S.emulate_case("f16", e), y, "emulation of the probe", sums=True)
    # the three-product emulation of the contract agrees (no l l)
    gn, wr = torch.from_numpy(e["gn"]), torch.relu(torch.from_numpy(e["w"]))
    em = K.emulate(K.dgrad_op, gn, wr, gn.abs().amax(dim=(1, 2, 3, 4), keepdim=True), float(wr.max())).numpy()
    T.same_bits(np.where(inmap, m * em, 0.0), y, "f16x2_contract.emulate", sums=True)


def test_probe_placement_over_window_sizes():
    at = S.PROBE_W_AT
    assert {(tz * 9 + ty * 3 + tx) for _, _, tz, ty, tx in at.values()} >= {0, 26} and any(0 < tz * 9 + ty * 3 + tx < 26 for _, _, tz, ty, tx in at.values())
    assert {ci % 16 // 8 for ci, *_ in at.values()} == {0, 1} and {ci // 16 % 2 for ci, *_ in at.values()} == {0, 1}
    assert any(co >= 32 for _, co, *_ in at.values())


# ------------------------------------------------------------------ the unmutated emulation stays within its bound
@pytest.mark.parametrize("kind,c,family", [(k, c, f) for k in KINDS for c, f in S.bounded_table(k)], ids=kid)
def test_bounded_case(kind, c, family):
    e, y, b, live = S.bounded_reference(kind, c, family)
    amax = np.abs(e["gn"]).reshape(c.P, -1).max(1)
    if family == "zero":
        assert not e["gn"].any() and not live.any()
    elif not family.startswith("at_bound"):
        assert c.P == 1 or amax.max() / amax.min() > 2.0 ** 40                      # the per-peak magnitudes are spread
        assert live.any()
    r = S.held(S.emulate_case(kind, e), y, b, live, S.case_id(c) + " " + family)
    print("prm small emulation: %s %s %s %.4f" % (kind, S.case_id(c), family, r))
    assert r <= 1.0, r


def test_clamp_edge():
    e, y, b, live = S.clamp_reference()
    c = S.CLAMP_CASE
    amax = np.abs(e["gn"]).reshape(c.P, -1).max(1)
    for p, k in S.CLAMP_PEAKS.items():
        assert amax[p] == 2.0 ** k and live[p].any()
    assert sorted(S.CLAMP_PEAKS.values()) == [-125, -112, -100] and amax[S.CLAMP_ZERO_PEAK] == 0 and not live[S.CLAMP_ZERO_PEAK].any()
    s = [K.scale_of(a)[0] for a in amax]
    assert s[2] == 2.0 ** 114 and s[4] == s[6] == s[S.CLAMP_ZERO_PEAK] == 2.0 ** 125          # 2^-100 is not clamped, the others are
    assert all(amax[p] > 1e-9 for p in range(c.P) if p not in S.CLAMP_PEAKS and p != S.CLAMP_ZERO_PEAK)
    # 1 / s <= A_eff 2^-14, the one place the contract's derivation uses the scale
    for p in range(c.P):
        assert 1.0 / s[p] <= max(amax[p], S.A_EFF_MIN) * 2.0 ** -14
    # below 2^-126 an fp32 result rounds to a multiple of 2^-149: the cut's own absolute term of E covers the epilogue's three roundings
    m, inmap = S.multiplier(e)
    assert np.abs(m[inmap]).min() >= 1.0
    Sb = S.f16_terms(e)[2].numpy()
    for p in (4, 6):
        gain = np.abs(m[p])[live[p]]
        assert np.all(gain * K.C2 * 2.0 ** -39 * S.A_EFF_MIN * Sb[p][live[p]] >= (1 + gain) * 2.0 ** -150)
        assert np.abs(y[p]).max() < 2.0 ** -100
    # E at A_eff differs from E at A on the clamped peaks only
    b0 = S.f16_bound(e, y)[0]
    assert all(np.array_equal(b0[p], b[p]) == (p not in (4, 6, S.CLAMP_ZERO_PEAK)) or not live[p].any() for p in range(c.P))
    got = S.emulate_case("f16", e)
    r = S.held(got, y, b, live, "clamp edge")
    rp = {p: S.held(got[p:p + 1], y[p:p + 1], b[p:p + 1], live[p:p + 1], "clamp edge") for p in S.CLAMP_PEAKS}
    print("prm small emulation: clamp edge %.4f, the tiny peaks %s" % (r, rp))
    assert r <= 1.0, r


# ------------------------------------------------------------------ every seeded defect is caught
def caught(kind, e, y, defect, what):
    with pytest.raises(AssertionError):
        T.same_bits(S.emulate_case(kind, e, defect), y, what, sums=True)


@pytest.mark.parametrize("defect", sorted(S.DEFECTS), ids=str)
def test_defect_is_caught_wherever_it_applies(defect):
    n = 0
    for kind in S.DEFECTS[defect]:
        for c in S.CASES[kind]:
            if S.applies(defect, kind, c):
                e, y, _ = S.exact_reference(kind, c)
                caught(kind, e, y, defect, "%s on %s %s" % (defect, kind, S.case_id(c)))
                n += 1
        if kind == "f16":
            for win, which in ALL_PROBES:
                if S.applies(defect, kind, S.PROBE_SHAPES[win], probe=which):
                    e, y, _ = S.probe_reference(win, which)
                    caught(kind, e, y, defect, "%s on the %s probe, win %d" % (defect, which, win))
                    n += 1
    assert n >= 1, "the defect applies to no case"
    assert set(S.DEFECTS[defect]) <= set(KINDS)


def test_every_listed_defect_exists():
    assert len(S.DEFECTS) == 15
    with pytest.raises(AssertionError):
        S.emulate("f32", *(S.exact_inputs("f32", S.F32_CASES[0])[k] for k in ("gn", "w", "full", "off", "origin")), defect="lo_half")
