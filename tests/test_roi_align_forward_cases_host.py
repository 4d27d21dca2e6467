"""CPU: the case table of tests/roi_align_forward_cases.py, without a GPU.

 (a) the fp64 reference against the C oracle (oracle.roi_align_3d_forward: fp32, the reference's operation order) on every case: every
     element inside the derived bound, exact zeros exact - the oracle is one of the orders the bound covers;
 (b) coverage, from roi_align_forward_cases.route() - launch() and the kernels' tier rules restated on the host: every code path of the
     fp32 forward under every hand-over kind is reached by a RoI of a named case, the two-channel loop of v3 ends both evenly and raggedly (a partial iteration after a full one),
     waves get two, one and no channel of a chunk, and the adaptive case really lands on the register-tap tiers.  A moved threshold in the
     kernel file has to be moved in route() too, and then shows here as a missing label, not silently on the GPU;
 (c) the bound separates: eight wrong forwards each leave it on a case the right one passes, and for each it is recorded whether the
     suite's older criterion (max |got - ref| <= 1e-5 * max |f|) would have accepted it;
 (d) the refusals of the C entry points, which are made before a device pointer is followed and need no GPU."""
import collections
import ctypes as C

import numpy as np
import pytest

import roi_align_backward_cases as T
import roi_align_forward_cases as Fc

# (label, hand-over kind) -> the case that is in the table to reach it
REACHED_BY = {
    ("v3.w4.dual", "marks"): "marks_c64", ("v3.w4.single", "marks"): "marks_c64", ("v3.w2", "marks"): "marks_c64",
    ("v3.w1", "marks"): "marks_c64", ("sep.zero", "marks"): "marks_c64", ("sep.reg_staged", "marks"): "marks_c64",
    ("sep.reg_globalx", "marks"): "marks_c64", ("sep.coop", "marks"): "marks_c64", ("sep.exact", "marks"): "marks_c64",
    ("v3.w4.dual", "predicate"): "pred_c43", ("v3.w4.single", "predicate"): "pred_c37", ("v3.w2", "predicate"): "pred_c40",
    ("v3.w1", "predicate"): "pred_c8", ("sep.zero", "predicate"): "pred_c8", ("sep.reg_staged", "predicate"): "pred_c37",
    ("sep.reg_globalx", "predicate"): "pred_c40", ("sep.coop", "predicate"): "pred_c37", ("sep.exact", "predicate"): "pred_c8",
    ("sep.zero", "none"): "bins3", ("sep.reg_staged", "none"): "adaptive_222", ("sep.reg_globalx", "none"): "adaptive_222",
    ("sep.coop", "none"): "adaptive_222", ("sep.exact", "none"): "adaptive_tabled", ("sep.untabled", "none"): "adaptive_untabled",
    ("sep.generic_staged", "none"): "noncubic",
}


def test_the_table_is_the_one_the_tests_are_written_for():
    for c in Fc.CASES:
        B, Cc, S, H, W = c.shape
        assert S <= 16 and H <= 16 and W <= 40 and Cc <= 64 and c.R <= 64
        r, f = Fc.rois(c), Fc.features(c)
        assert r.shape == (c.R, 7) and f.shape == c.shape and f.dtype == np.float32
        assert np.isfinite(r).all() and np.isfinite(f).all()
        assert (r[:, 0] >= 0).all() and (r[:, 0] < B).all() and (r[:, 0] == np.floor(r[:, 0])).all()
        # the last two channels are quiet: below 1e-3 of the loudest channel, where a tolerance relative to max |f| sees nothing
        rms = np.sqrt((f.astype(np.float64) ** 2).mean(axis=(0, 2, 3, 4)))
        assert (rms[-2:] < 1e-3 * rms.max()).all(), (c.id, rms)
        assert Cc < 8 or rms[:-2].max() / rms[:-2].min() > 2, (c.id, rms)
    z = (Fc.features(Fc.BY_ID["pred_c37"]) == 0).mean()
    assert 0.07 < z < 0.13, z
    assert {c.shape[1] for c in Fc.V3_CASES} == {64, 40, 37, 8, 43}
    assert Fc.BY_ID[Fc.SHIPPED] in Fc.V3_CASES
    big = Fc.BY_ID["marks_c64"]
    assert set(Fc.rois(big)[:, 0]) == {0.0, 1.0}
    same = (Fc.rois(big)[:, None, :] == Fc.rois(big)[None, :, :]).all(2).sum(1)
    assert same.max() >= 2                                                           # a duplicated RoI


@pytest.mark.parametrize("c", Fc.CASES, ids=Fc.case_id)
def test_reference_against_the_c_oracle(c):
    res = Fc.reference_of(c)
    v = Fc.compare(Fc.oracle_of(c), res)
    print("%s: oracle %s; largest n_o %d" % (c.id, Fc.describe(v), res.n.max()))
    assert v.outside == 0 and v.nonzero == 0, Fc.describe(v)
    assert (res.A > 0).any() and np.abs(res.ref).max() > 0
    assert (np.abs(res.ref) <= res.A * (1 + 1e-12)).all()
    assert ((res.A > 0) <= (res.n >= 8)).all()
    # the smallest live A_o is far above the range where an fp32 product would leave the normal numbers
    assert res.A[res.A > 0].min() > 1e-20


def test_every_route_under_every_handover_is_reached():
    assert set(REACHED_BY) == set(Fc.REQUIRED)
    reached = collections.defaultdict(set)
    for c in Fc.CASES:
        for rt in Fc.routes_of(c):
            reached[(rt.label, rt.handover)].add(c.id)
    for key in sorted(Fc.REQUIRED):
        print("%-20s %-10s %s" % (key + (REACHED_BY[key] + " (also: " + ", ".join(sorted(reached[key] - {REACHED_BY[key]})) + ")",)))
    missing = sorted(k for k in Fc.REQUIRED if REACHED_BY[k] not in reached[k])
    assert not missing, missing
    assert set(reached) == set(Fc.REQUIRED), sorted(set(reached) - set(Fc.REQUIRED))     # and route() knows no label beyond the list


@pytest.mark.parametrize("c", Fc.V3_CASES, ids=Fc.case_id)
def test_the_sized_rois_land_where_they_were_sized_for(c):
    """the sub-volumes of the issue's table (4^3, 8^3, 12^3, 16^3, 3x4x36, 6x7x40, 12x14x36, 16x16x32), through route()"""
    rts = Fc.routes_of(c)
    assert tuple(rt.label for rt in rts[:8]) == Fc.ENGINEERED
    assert [rt.sub for rt in rts[:8]] == [64, 512, 1728, 4096, 432, 1680, 6048, 8192]
    assert [rt.nw for rt in rts[:4]] == [4, 4, 2, 1] and [rt.dual for rt in rts[:4]] == [True, False, False, False]
    kind = "marks" if c.id == "marks_c64" else "predicate"
    assert all(rt.handover == kind for rt in rts)


def test_chunks_waves_and_loop_endings():
    by = {c.id: Fc.routes_of(c) for c in Fc.V3_CASES}
    # markers: C = 64 with few RoIs gives complement chunks of 8; a small RoI is ONE workgroup, a medium one a workgroup per 8 channels
    m = by["marks_c64"]
    assert m[4].chunks == [(8 * k, 8 * k + 8) for k in range(8)]
    assert m[0].chunks == [(0, 64)] and m[2].chunks == m[3].chunks == [(8 * k, 8 * k + 8) for k in range(8)]
    # predicate: 32 channels per v3 workgroup, complement chunks of 5 (C = 40, 37) or one of 8
    assert by["pred_c40"][0].chunks == [(0, 32), (32, 40)] and by["pred_c37"][0].chunks == [(0, 32), (32, 37)]
    assert by["pred_c37"][4].chunks[-1] == (35, 37) and by["pred_c40"][4].chunks[-1] == (35, 40) and by["pred_c8"][4].chunks == [(0, 8)]
    # a wave gets two, one or no channel of a chunk: v3 (two and one) and the complement's last chunk (one and none)
    assert {1, 2} <= set(by["pred_c37"][0].wave_channels) and {0, 1, 2} <= set(by["pred_c37"][4].wave_channels)
    # the two-channel loop: even endings under both hand-over kinds.  A ragged one - a partial iteration AFTER a full one, the
    # `if (!more) first = true` branch - needs a wave with 3, 5, .. channels: a chunk that is no multiple of 8 channels, which the markers'
    # rule (C % 32 == 0) excludes, so it exists under the predicate alone; C = 43 (chunks 32 + 11: waves with 3, 3, 3, 2 channels) reaches
    # it.  C = 37 (32 + 5: 2, 1, 1, 1) only has waves whose single iteration is partial, which is the ordinary first iteration.
    dual = {cid: [rt for rt in rts if rt.dual] for cid, rts in by.items()}
    assert all(dual.values())
    assert all(rt.even and not rt.ragged and not rt.lone for cid in ("marks_c64", "pred_c40", "pred_c8") for rt in dual[cid])
    assert all(rt.even and rt.lone and not rt.ragged and rt.wave_channels == [1, 2, 8] for rt in dual["pred_c37"])
    assert by["pred_c43"][0].chunks == [(0, 32), (32, 43)]
    assert all(rt.ragged and rt.even and not rt.lone and rt.wave_channels == [2, 3, 8] for rt in dual["pred_c43"])
    assert len(dual["pred_c43"]) >= 3 and {int(Fc.rois(Fc.BY_ID["pred_c43"])[i, 0]) for i, rt in enumerate(by["pred_c43"]) if rt.dual} == {0, 1}
    assert not any(rt.ragged or rt.even or rt.lone for rts in by.values() for rt in rts if not rt.dual)


def test_adaptive_cases_reach_their_grids():
    grids = [rt.grid for rt in Fc.routes_of(Fc.BY_ID["adaptive_222"])]
    assert set(grids) == {(2, 2, 2)}                                  # ratio 0, and yet reg_taps for every RoI, small and large
    subs = [rt.sub for rt in Fc.routes_of(Fc.BY_ID["adaptive_222"])]
    assert min(subs) <= 64 and max(subs) >= 2000
    grids = [rt.grid for rt in Fc.routes_of(Fc.BY_ID["adaptive_tabled"])]
    assert min(k for g in grids for k in g) == 1 and max(k for g in grids for k in g) == 9
    assert any(len(set(g)) == 3 for g in grids)
    rts = Fc.routes_of(Fc.BY_ID["adaptive_untabled"])
    assert [rt.label == "sep.untabled" for rt in rts] == [True, True, False, False] and max(k for rt in rts for k in rt.grid) == 12


def test_the_forward_keeps_the_z_band():
    """samples with z in [-1, -0.1): dropped by the backward's rule, kept by the forward's - the table has them, valid, next to valid y, x"""
    for cid in ("marks_c64", "pred_c37", "adaptive_222"):
        c = Fc.BY_ID[cid]
        n = 0
        for g in Fc.reference_of(c).geoms:
            z = g.axes[0]
            band = (z.raw >= -1.0) & (z.raw < -0.1)
            assert z.valid[band].all()
            n += int(band.sum()) if g.axes[1].valid.any() and g.axes[2].valid.any() else 0
        assert n >= 2, (cid, n)
    # every class of sample on every axis of the largest case
    c = Fc.BY_ID["marks_c64"]
    for a in range(3):
        raw = np.concatenate([g.axes[a].raw.ravel() for g in Fc.reference_of(c).geoms])
        valid = np.concatenate([g.axes[a].valid.ravel() for g in Fc.reference_of(c).geoms])
        clamped = np.concatenate([(g.axes[a].lo == g.axes[a].hi).ravel() for g in Fc.reference_of(c).geoms])
        dim = c.shape[2 + a]
        assert (raw < -1.0).any() and not valid[raw < -1.0].any() and (raw > dim).any() and not valid[raw > dim].any()
        assert (valid & clamped).any() and (valid & (raw <= 0)).any() and (valid & ~clamped & (raw > 0)).any()


# ---------------------------------------------------------------------------------------------- sensitivity
def _variant(**kw):
    return lambda c: Fc.reference(Fc.features(c), Fc.rois(c), c.shape, c.bins, c.scale, c.ratio, **kw).ref


def _natural_order(c):
    """the values written in the tensor's own (ps, ph, pw) order instead of the kernel's (ph, pw, ps)"""
    return np.ascontiguousarray(Fc.reference_of(c).ref.transpose(0, 1, 4, 2, 3))


def _stale_channel(c):
    """the last channel's result is the one before it: a stale LDS buffer on the last, ragged channel of a wave"""
    out = Fc.oracle_of(c).astype(np.float64).reshape(Fc.reference_of(c).ref.shape).copy()
    out[:, -1] = out[:, -2]
    return out


def _quiet_channel(c):
    """the quietest channel off by 1 % of its own magnitude"""
    out = Fc.oracle_of(c).astype(np.float64).reshape(Fc.reference_of(c).ref.shape).copy()
    out[:, -1] *= 1.01
    return out


# name -> (the wrong forward, does the older criterion 1e-5 * max |f| accept it?)
WRONG = {
    "z_limit": (_variant(z_limit=-0.1), False),
    "natural_order": (_natural_order, False),
    "count": (_variant(count_plus=1), False),
    "batch": (_variant(ignore_batch=True), False),
    "hi_is_lo": (_variant(hi_is_lo=True), False),
    "fourth_tap": (_variant(drop_fourth_tap=True), False),
    "stale_channel": (_stale_channel, True),
    "quiet_channel": (_quiet_channel, True),
}


@pytest.mark.parametrize("what", list(WRONG))
def test_the_bound_tells_a_wrong_forward_from_the_right_one(what):
    c = Fc.BY_ID["pred_c37"]
    res = Fc.reference_of(c)
    right = Fc.compare(Fc.oracle_of(c), res)
    assert right.outside == 0 and right.nonzero == 0 and Fc.old_criterion(Fc.oracle_of(c), res, Fc.features(c))
    make, old_accepts = WRONG[what]
    wrong = make(c)
    v = Fc.compare(wrong, res)
    old = Fc.old_criterion(wrong, res, Fc.features(c))
    print("%-14s new: %s; 1e-5 * max |f| %s it" % (what, Fc.describe(v), "ACCEPTS" if old else "rejects"))
    assert v.outside >= 100, (what, Fc.describe(v))
    assert old == old_accepts, (what, old)


def test_a_stale_last_channel_shows_where_the_loop_is_ragged():
    """the same model on the case whose two-channel loops end with a partial iteration after a full one (channel 42 is the third, lone
    channel of wave 2 in the chunk 32 .. 42)"""
    c = Fc.BY_ID["pred_c43"]
    assert any(rt.ragged for rt in Fc.routes_of(c))
    res = Fc.reference_of(c)
    wrong = _stale_channel(c)
    v = Fc.compare(wrong, res)
    print("stale_channel on pred_c43: %s" % Fc.describe(v))
    assert v.outside >= 100 and Fc.old_criterion(wrong, res, Fc.features(c))


def test_the_older_criterion_accepted_at_least_two_of_them():
    assert sum(accepts for _, accepts in WRONG.values()) >= 2


def test_the_output_order_shows_on_non_cubic_bins():
    c = Fc.BY_ID["noncubic"]
    v = Fc.compare(_natural_order(c), Fc.reference_of(c))
    assert v.outside >= 100, Fc.describe(v)


# ---------------------------------------------------------------------------------------------- refusals of the C entry points
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


FAKE = C.c_void_p(4096)          # a non-NULL "device pointer" that a refusing call never follows


def _call(L, name, bins=(7, 7, 7), ratio=2, R=1, cols=7, shape=(1, 4, 6, 7, 8), feat=FAKE, rois=FAKE, out=FAKE):
    args = [bins[0], bins[1], bins[2], C.c_float(0.125), ratio, feat] + list(shape) + [rois, R, cols, out]
    if name == "m3d_roi_align3d_forward_ws":
        args += [None, C.c_size_t(0)]
    return getattr(L, name)(*args, None)


@pytest.mark.parametrize("name", ["m3d_roi_align3d_forward", "m3d_roi_align3d_forward_ws", "m3d_roi_align3d_forward_exact"])
def test_refusals_without_gpu(L, name):
    q = T.REFUSED
    assert max(q["bins"]) * q["ratio"] > Fc.K_MAX_TABLE
    assert _call(L, name, bins=q["bins"], ratio=q["ratio"], shape=q["shape"]) == Fc.M3D_EUNSUPPORTED     # a FIXED ratio beyond the tables
    assert _call(L, name, bins=(8, 8, 8), ratio=9) == Fc.M3D_EUNSUPPORTED
    for cols in (5, 6, 8, 0):
        assert _call(L, name, cols=cols) == Fc.M3D_EINVAL, cols                                          # roi_align_cuda_3d.c:19-22
    assert _call(L, name, R=0) == 0 and _call(L, name, R=0, feat=None, rois=None, out=None) == 0         # nothing to do: OK
    assert _call(L, name, R=-1) == Fc.M3D_EINVAL
    for null in ("feat", "rois", "out"):
        assert _call(L, name, **{null: None}) == Fc.M3D_EINVAL, null
    for bad in ((0, 4, 6, 7, 8), (1, 0, 6, 7, 8), (1, 4, 0, 7, 8), (1, 4, 6, 0, 8), (1, 4, 6, 7, 0)):
        assert _call(L, name, shape=bad) == Fc.M3D_EINVAL, bad
    assert _call(L, name, bins=(7, 0, 7)) == Fc.M3D_EINVAL
    assert _call(L, name, cols=5, R=0) == Fc.M3D_EINVAL                                                  # the column check comes first
