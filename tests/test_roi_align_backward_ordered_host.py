"""CPU: the ordered RoIAlign3D backward without a GPU (tests/roi_align_backward_ordered_cases.py; csrc/roi_align3d_bwd.hip).

 (a) the NumPy fp32 restatement of the kernel's operation order is inside the derived bound (K = 8) on every case of the table the
     ordered path accepts and on the extra cases, exact zeros exact;
 (b) with that K the five wrong backwards of tests/test_roi_align_backward_cases_host.py are still rejected on `shipped` and `noncubic_a`;
 (c) the extra cases reach what they are for - tiles, empty lists, short and ragged shares - proved from the sample tables and the
     restated launch plan;
 (d) every refusal of m3d_roi_align3d_backward_ordered returns its code before a pointer is followed; the mode switch of m3d.compat."""
import ctypes as C
import sys

import numpy as np
import pytest

import roi_align_backward_cases as T
import roi_align_backward_ordered_cases as Q
from test_roi_align_backward_cases_host import WRONG

EINVAL, EUNSUPPORTED = -1, -4
ALL = Q.ACCEPTED + Q.EXTRA


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("c", ALL, ids=T.case_id)
def test_restatement_is_inside_the_bound(c):
    res = Q.reference_of(c)
    got = Q.ordered_backward(Q.top(c), Q.rois(c), c.shape, c.bins, c.scale, c.ratio)
    assert got.dtype == np.float32 and got.shape == c.shape and np.isfinite(got).all()
    v = Q.compare(got, res)
    print("%s: restatement %s; nw %d" % (c.id, T.describe(v), Q.plan(c.bins, c.shape[2:]).nw))
    assert v.outside == 0 and v.nonzero == 0, T.describe(v)
    assert c.R == 0 or ((res.A > 0).any() and np.abs(got).max() > 0)


def test_the_accepted_cases_are_all_but_the_untabled_one():
    assert len(Q.ACCEPTED) == len(T.CASES) - 1
    for c in T.CASES:
        beyond = any(T.untabled(g, c.bins) for g in T.reference_of(c).geoms)
        assert beyond == (c not in Q.ACCEPTED), c.id
    # the derivation's premise: a weight is zero or >= 2^-24, so no product underflows
    for c in ALL:
        for g in Q.reference_of(c).geoms:
            for t in g.axes:
                w = np.concatenate([t.l[t.valid], t.h[t.valid]])
                assert not ((w != 0) & (w < 2.0 ** -24)).any(), c.id
                assert g.count <= 729


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("cid", ["shipped", "noncubic_a"])
@pytest.mark.parametrize("what", list(WRONG))
def test_the_bound_still_rejects_the_wrong_backwards(cid, what):
    assert len(WRONG) == 5
    c = T.BY_ID[cid]
    res = T.reference_of(c)
    wrong = T.reference(T.top(c), T.rois(c), c.shape, c.bins, c.scale, c.ratio, **WRONG[what]).grad
    v = Q.compare(wrong, res)
    print("%s, %s: %s" % (cid, what, T.describe(v)))
    assert v.outside >= 100, (what, T.describe(v))


# ---------------------------------------------------------------------------------------------------------------- (c)
def _boxes(c):
    """per RoI the voxel box (z0, z1, y0, y1, x0, x1) its valid samples reach, or None"""
    out = []
    for g in Q.reference_of(c).geoms:
        r = [Q.reach(t) for t in g.axes]
        out.append(None if any(x is None for x in r) else tuple(v for lohi in r for v in lohi))
    return out


def _tiles_met(box, pl):
    return {(z, y, x) for z in range(box[0] // pl.tile[0], box[1] // pl.tile[0] + 1)
            for y in range(box[2] // pl.tile[1], box[3] // pl.tile[1] + 1) for x in range(box[4] // pl.tile[2], box[5] // pl.tile[2] + 1)}


def test_plan_of_the_shapes_that_matter():
    p = Q.plan((7, 7, 7), (16, 16, 16))                       # the box head's training shape: one 16 KB tile, three waves
    assert p.tile == (16, 16, 16) and p.ntiles == (1, 1, 1) and p.stage and p.nw == 3 and 4 * p.per_wave * p.nw <= 64 * 1024
    p = Q.plan((7, 7, 7), (16, 64, 64))                       # the soma tile's map
    assert p.ntiles == (1, 4, 4) and p.nw == 3
    p = Q.plan((64, 64, 64), (16, 16, 16))                    # the largest tables: one wave still fits
    assert not p.stage and p.nw == 1 and 4 * p.per_wave <= Q.LDS_BUDGET
    p = Q.plan((14, 14, 14), (16, 16, 16))                    # more than 1024 bins: top is read from global memory
    assert not p.stage and p.nw >= 2
    for c in ALL:
        p = Q.plan(c.bins, c.shape[2:])
        assert 1 <= p.nw <= 4 and 4 * p.per_wave * p.nw <= Q.LDS_BUDGET and p.per_wave % 4 == 0


def test_tiled_case_reaches_the_tiling():
    c = Q.EXTRA_BY_ID["tiled"]
    pl = Q.plan(c.bins, c.shape[2:])
    dims = c.shape[2:]
    assert pl.ntiles == (2, 2, 3) and pl.nw == 3
    assert all(d > t and d % t != 0 for d, t in zip(dims, pl.tile))               # larger on every axis, no multiple
    assert dims[0] * dims[1] * dims[2] < 10 ** 5
    boxes = _boxes(c)
    assert all(b is not None for b in boxes[:7])
    met = [_tiles_met(b, pl) for b in boxes]
    assert len(met[0]) == 12                                                      # covers all tiles
    assert met[1] == {(0, 0, 0)} and met[6] == {(1, 1, 2)}                        # inside one tile: the first, the last (ragged) one
    assert met[2] == {(0, 0, 0), (0, 0, 1)} and met[3] == {(0, 0, 0), (0, 1, 0)} and met[4] == {(0, 0, 0), (1, 0, 0)}
    assert len(met[5]) == 12 and boxes[5][4] > 0                                  # straddles every border without starting at the map's
    # every tile is met by some RoI and missed by some RoI (culling runs both ways)
    for t in met[0]:
        assert sum(t in m for m in met) >= 2 and any(t not in m for m in met), t
    # the shares of the 13-entry list: 4, 4, 5
    assert [i1 - i0 for i0, i1 in Q.shares(c.R, pl.nw)] == [4, 4, 5]


def test_bucket_cases_reach_the_lists():
    c = Q.EXTRA_BY_ID["empty_middle"]
    b = Q.rois(c)[:, 0]
    assert c.shape[0] == 3 and (b == 0).sum() >= 3 and (b == 1).sum() == 0 and (b == 2).sum() >= 3
    assert (np.diff(b) < 0).any()                                                 # not sorted by image: the compaction has to be one
    assert not Q.reference_of(c).A[1].any() and Q.reference_of(c).A[0].any() and Q.reference_of(c).A[2].any()
    c = Q.EXTRA_BY_ID["last_image"]
    assert (Q.rois(c)[:, 0] == c.shape[0] - 1).all() and not Q.reference_of(c).A[0].any() and Q.reference_of(c).A[1].any()
    c = Q.EXTRA_BY_ID["short_lists"]
    nw = Q.plan(c.bins, c.shape[2:]).nw
    lists = Q.image_lists(Q.reference_of(c).geoms, c.shape[0])
    assert nw == 4 and [len(l) for l in lists] == [2, 7]
    assert lists[0] == [3, 6]
    assert [i1 - i0 for i0, i1 in Q.shares(2, nw)] == [0, 1, 0, 1]                # fewer RoIs than waves: two waves have none
    assert [i1 - i0 for i0, i1 in Q.shares(7, nw)] == [1, 2, 2, 2]                # no multiple of the waves
    assert all(bx is not None for bx in _boxes(c))                                # every one of them contributes
    c = Q.EXTRA_BY_ID["no_rois"]
    assert c.R == 0 and Q.rois(c).shape == (0, 7) and not Q.reference_of(c).A.any()
    c = T.BY_ID["many_rois"]
    assert c.R > 256 * 8                                                          # several 256-RoI rounds of the compaction


def test_restatement_roi_order_matters_only_in_the_last_bits():
    """the list order is part of the operation order: the RoIs reversed give another fp32 result on `shipped`, inside the bound all the same"""
    c = T.BY_ID["shipped"]
    a = Q.ordered_backward(Q.top(c), Q.rois(c), c.shape, c.bins, c.scale, c.ratio)
    rev = list(range(c.R))[::-1]
    b = Q.ordered_backward(Q.top(c), Q.rois(c), c.shape, c.bins, c.scale, c.ratio, order=rev)
    assert not np.array_equal(a, b)
    v = Q.compare(b, Q.reference_of(c))
    assert v.outside == 0 and v.nonzero == 0


# ---------------------------------------------------------------------------------------------------------------- (d)
def _call(L, bins=(7, 7, 7), ratio=2, top=0x1000, rois=0x2000, R=4, cols=7, grad=0x3000, shape=(2, 4, 6, 7, 8), ws=0x4000, wsb=None):
    B, Cc, S, H, W = shape
    if wsb is None:
        wsb = L.m3d_roi_align3d_backward_ordered_workspace_bytes(max(R, 0), max(B, 0))
    return L.m3d_roi_align3d_backward_ordered(bins[0], bins[1], bins[2], C.c_float(0.125), ratio, C.c_void_p(top), C.c_void_p(rois), R, cols,
                                              C.c_void_p(grad), B, Cc, S, H, W, C.c_void_p(ws), C.c_size_t(wsb), None)


def test_refusals_without_a_gpu(L):
    """every call below is refused before a pointer is followed (the pointers are not memory) or anything is launched"""
    need = L.m3d_roi_align3d_backward_ordered_workspace_bytes(4, 2)
    assert need >= 4 * (1 + 2 * 2 + 7 * 4) and L.m3d_roi_align3d_backward_ordered_workspace_bytes(0, 1) >= 4
    assert need % 4 == 0 and L.m3d_roi_align3d_backward_ordered_workspace_bytes(1000, 2) > need
    assert _call(L, top=0) == EINVAL and _call(L, rois=0) == EINVAL and _call(L, grad=0) == EINVAL and _call(L, ws=0) == EINVAL
    assert _call(L, R=0, grad=0) == EINVAL                                        # the map is never empty: it is always written
    assert _call(L, R=0, ws=0) == EINVAL
    assert _call(L, cols=6) == EINVAL and _call(L, cols=8) == EINVAL
    assert _call(L, R=-1) == EINVAL
    for i in range(5):
        for bad in (0, -3):
            shape = [2, 4, 6, 7, 8]
            shape[i] = bad
            assert _call(L, shape=tuple(shape)) == EINVAL, shape
    for i in range(3):
        for bad in (0, -1):
            bins = [7, 7, 7]
            bins[i] = bad
            assert _call(L, bins=tuple(bins)) == EINVAL, bins
    assert _call(L, wsb=need - 1) == EINVAL and _call(L, wsb=0) == EINVAL
    # a fixed ratio beyond the tables: the rule of the atomic backward, checked as REFUSED of the case table is
    q = T.REFUSED
    assert max(q["bins"]) * q["ratio"] > T.K_MAX_TABLE
    assert _call(L, bins=q["bins"], ratio=q["ratio"], R=q["rois"].shape[0], shape=q["shape"]) == EUNSUPPORTED
    assert _call(L, bins=(7, 7, 10), ratio=7) == EUNSUPPORTED and _call(L, bins=(33, 2, 2), ratio=2) == EUNSUPPORTED
    assert _call(L, bins=(65, 7, 7), ratio=0) == EUNSUPPORTED                      # adaptive: the grid is >= 1, so 65 bins never fit
    # argument errors come first
    assert _call(L, bins=q["bins"], ratio=q["ratio"], cols=5) == EINVAL


def test_mode_switch():
    import m3d
    import m3d.compat as K
    assert callable(m3d.roi_align3d_backward_ordered) and "roi_align3d_backward_ordered" in m3d.ops.__all__
    assert K.get_roi_align_backward() == "atomic"
    for bad in ("gather", "", None, "Ordered"):
        with pytest.raises(ValueError):
            K.set_roi_align_backward(bad)
        assert K.get_roi_align_backward() == "atomic"
    try:
        assert K.set_roi_align_backward("ordered") == "atomic" and K.get_roi_align_backward() == "ordered"
        assert K.set_roi_align_backward("ordered") == "ordered"
        assert K.set_roi_align_backward("atomic") == "ordered" and K.get_roi_align_backward() == "atomic"
    finally:
        K.set_roi_align_backward("atomic")


def test_install_leaves_the_mode_alone():
    import torch.nn.functional as F
    import m3d.compat as K
    conv, lin, bn = F.conv3d, F.linear, F.batch_norm
    modules = dict(sys.modules)                      # install() registers stand-in packages (modeling, utils, ...): put them away again
    try:
        K.install()
        assert K.get_roi_align_backward() == "atomic"
        K.set_roi_align_backward("ordered")
        K.install()
        assert K.get_roi_align_backward() == "ordered"
    finally:
        K.set_roi_align_backward("atomic")
        K.uninstall_batch_norm()
        K.uninstall_conv3d()
        K.uninstall_linear()
        F.conv3d, F.linear, F.batch_norm = conv, lin, bn
        for k in [k for k in sys.modules if k not in modules]:
            del sys.modules[k]
