"""CPU: the case table of tests/roi_align_backward_cases.py, without a GPU.

 (a) the fp64 reference against the C oracle (oracle.roi_align_3d_backward: fp32, sequential order) on every case: every element inside
     the derived bound, exact zeros exact - the oracle is one of the orders the bound covers;
 (b) the table reaches what it is for, computed from the reference's own sample tables and launch()'s chunk rule restated in
     roi_align_backward_cases.chunk_sizes: a moved table limit, chunk threshold or RoI stops the test here, not silently on the GPU;
 (c) the bound separates: five wrong backwards (variants of the reference, not of the kernel) each leave it on `shipped` and on
     `noncubic_a`."""
import numpy as np
import pytest

import oracle as O
import roi_align_backward_cases as T

# id -> (channels per chunk, the least trips of the `e += blockDim.x` loop in the largest chunk, RoIs on the untabled path)
EXPECT = {
    "shipped": ([10, 10, 10, 7], 2, 0),
    "wide_c": ([16] * 16, 2, 0),
    "narrow_c": ([5], 1, 0),
    "many_rois": ([24], 1, 0),
    "noncubic_a": ([9], 1, 0),
    "noncubic_b": ([9], 1, 0),
    "table_edge": ([4], 2, 0),
    "adaptive_tabled": ([6], 2, 0),
    "adaptive_untabled": ([3], 2, 2),
    "avg_wrapper": ([8], 2, 0),
}


def test_the_table_is_the_one_the_tests_are_written_for():
    assert [c.id for c in T.CASES] == list(EXPECT)
    for c in T.CASES:
        assert T.rois(c).shape == (c.R, 7) and T.top(c).shape == (c.R, c.shape[1]) + c.bins
        r = T.rois(c)
        assert np.isfinite(r).all() and (r[:, 0] >= 0).all() and (r[:, 0] < c.shape[0]).all() and (r[:, 0] == np.floor(r[:, 0])).all()
        # a per-channel scale: the channels' magnitudes differ, so a channel mix-up cannot hide
        rms = np.sqrt((T.top(c).astype(np.float64) ** 2).mean(axis=(0, 2, 3, 4)))
        assert rms.max() / rms.min() > 2 or c.shape[1] < 8, (c.id, rms)
    z = (T.top(T.BY_ID["shipped"]) == 0).mean()
    assert 0.07 < z < 0.13, z
    assert T.BY_ID["many_rois"].R >= 2048


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_reference_against_the_c_oracle(c):
    res = T.reference_of(c)
    got = O.roi_align_3d_backward(T.top(c), T.rois(c), c.shape, *c.bins, c.scale, c.ratio)
    v = T.compare(got, res)
    print("%s: oracle %s; largest n_e %d" % (c.id, T.describe(v), res.n.max()))
    assert v.outside == 0 and v.nonzero == 0, T.describe(v)
    assert (res.A > 0).any() and np.abs(res.grad).max() > 0
    # the companions are what they say: |grad| <= A, an element with adds has n >= 1, and the adds of all elements are the valid samples' 8
    assert (np.abs(res.grad) <= res.A * (1 + 1e-12)).all()
    assert ((res.A > 0) <= (res.n >= 1)).all()
    adds = sum(8 * int(g.axes[0].valid.sum()) * int(g.axes[1].valid.sum()) * int(g.axes[2].valid.sum()) for g in res.geoms)
    assert res.n[:, 0].sum() == adds


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_chunks_loop_trips_and_table_path(c):
    sizes, trips, n_untabled = EXPECT[c.id]
    got = T.chunk_sizes(c.R, c.shape[1])
    assert got == sizes and sum(got) == c.shape[1], (c.id, got)
    bins = c.bins[0] * c.bins[1] * c.bins[2]
    assert (max(got) * bins + 255) // 256 >= trips
    if trips == 1:
        assert max(got) * bins <= 256
    geoms = T.reference_of(c).geoms
    assert sum(T.untabled(g, c.bins) for g in geoms) == n_untabled
    if c.ratio > 0:                             # a fixed ratio beyond the tables is refused, not computed
        assert max(c.bins) * c.ratio <= T.K_MAX_TABLE
    assert c.id != "table_edge" or max(c.bins) * c.ratio == T.K_MAX_TABLE - 1
    assert max(T.REFUSED["bins"]) * T.REFUSED["ratio"] > T.K_MAX_TABLE and T.REFUSED["ratio"] > 0


def _samples(c):
    """per axis (z, y, x) the raw coordinates and validity of every sample of every RoI, flat"""
    geoms = T.reference_of(c).geoms
    return [(np.concatenate([g.axes[a].raw.ravel() for g in geoms]), np.concatenate([g.axes[a].valid.ravel() for g in geoms]),
             np.concatenate([(g.axes[a].lo == g.axes[a].hi).ravel() for g in geoms])) for a in range(3)]


def test_shipped_has_every_class_of_sample():
    c = T.BY_ID["shipped"]
    dims = c.shape[2:]
    per_axis = _samples(c)
    for a, (raw, valid, clamped) in enumerate(per_axis):
        assert valid.any()
        assert (raw < -1.0).any() and not valid[raw < -1.0].any()                   # below -1: dropped
        assert (raw > dims[a]).any() and not valid[raw > dims[a]].any()             # above dim: dropped
        assert (valid & clamped).any()                                              # lo == hi == dim - 1: two adds to one address
        assert (valid & (raw <= 0)).any()                                           # c <= 0 -> 0
        assert (valid & ~clamped & (raw > 0)).any()
    zraw, zvalid, _ = per_axis[0]
    band = (zraw >= -1.0) & (zraw < -0.1)
    assert band.sum() >= 8 and not zvalid[band].any()                               # dropped backwards only
    for a in (1, 2):
        raw, valid, _ = per_axis[a]
        band = (raw >= -1.0) & (raw < -0.1)
        assert band.any() and valid[band].all()                                     # the same band stays valid on y and x
    # the z-band RoIs themselves: band samples on z whose y and x partners are valid, so the forward's rule would add there
    for g in T.reference_of(c).geoms[12:14]:
        z = g.axes[0]
        assert ((z.raw >= -1.0) & (z.raw < -0.1)).any() and g.axes[1].valid.any() and g.axes[2].valid.any()
    r = T.rois(c)
    assert set(r[:, 0]) == {0.0, 1.0}
    assert (r[:, 4] < r[:, 1]).any() and (r[:, 1:] == 4000).all(1).any()
    same = (r[:, None, :] == r[None, :, :]).all(2).sum(1)
    assert same.max() >= 3                                                          # the same RoI three times


def test_adaptive_cases_reach_their_grids():
    c = T.BY_ID["adaptive_tabled"]
    grids = [g.grid for g in T.reference_of(c).geoms]
    assert len({k for g in grids for k in g}) >= 3 and any(len(set(g)) == 3 for g in grids)
    assert min(k for g in grids for k in g) == 1 and max(k for g in grids for k in g) == 9
    c = T.BY_ID["adaptive_untabled"]
    grids = [g.grid for g in T.reference_of(c).geoms]
    assert any(all(k > 9 for k in g) for g in grids)
    assert any(sum(k > 9 for k in g) == 1 for g in grids)
    assert sum(all(k <= 9 for k in g) for g in grids) == 2
    assert max(k for g in grids for k in g) == 12


WRONG = {
    "z_limit": dict(z_limit=-1.0),
    "top_order": dict(top_forward_order=True),
    "count": dict(count_plus=1),
    "batch": dict(ignore_batch=True),
    "hi_is_lo": dict(hi_is_lo=True),
}


@pytest.mark.parametrize("cid", ["shipped", "noncubic_a"])
@pytest.mark.parametrize("what", list(WRONG))
def test_the_bound_tells_a_wrong_backward_from_the_right_one(cid, what):
    c = T.BY_ID[cid]
    res = T.reference_of(c)
    wrong = T.reference(T.top(c), T.rois(c), c.shape, c.bins, c.scale, c.ratio, **WRONG[what]).grad
    v = T.compare(wrong, res)
    print("%s, %s: %s" % (cid, what, T.describe(v)))
    assert v.outside >= 100, (what, T.describe(v))
    if what == "z_limit":
        # and the z-band RoIs alone already show it: the only difference is at z = 0, by those RoIs' batch items
        diff = np.abs(wrong - res.grad) > T.bound(res)
        assert diff[:, :, 0].any() and not diff[:, :, 1:].any()
