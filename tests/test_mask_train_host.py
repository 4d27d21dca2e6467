"""CPU: the NumPy restatement of the mask-branch training step (tests/mask_train_reference.py) reproduces the reference's own results
(tests/golden/mask_train.npz, made by gen_mask_train.py from add_mask_rcnn_blobs and mask_rcnn_losses) exactly, in both of its forms;
the footprint intervals the kernel computes equal the 1-D impulse definition of the resize for every length up to 256 at the shipped
resolution (and a sample up to the device's limit of 1024); the closed form equals "resize > 0" evaluated in fp64, contains what the
reference's fp32 resize gives, and differs from it only where that resize underflows - aimed at the lengths where it does; the C entry
points refuse bad arguments without a GPU; the configuration, the head's parameter names and Batch.gt_spots."""
import ctypes
import os
import types

import numpy as np
import pytest

import box_head_train_reference as BR
import mask_train_reference as MR

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_train.npz")
CASES = ["spot_small", "spot_big", "spot_3cls", "spot_nofg", "mask_small", "mask_nofg"]
LOSS_CASES = {"loss_spot": "spot_small", "loss_3cls": "spot_3cls"}
f32 = np.float32


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def case_inputs(g, name):
    """everything a golden case was made from, as a dict"""
    p = name + "_"
    n = g[p + "numbers"]
    mc = [int(v) for v in g[p + "mask_cfg"]]
    d = dict(box_cfg=BR.make_cfg(n[0], n[1], n[2], n[3], n[4], n[5], g[p + "weights"]), gt=g[p + "gt"], classes=g[p + "gt_classes"],
             crowd=g[p + "gt_crowd"], proposals=g[p + "proposals"], seed=int(g[p + "seed"]), M=mc[0], mode="mask" if mc[1] else "spot",
             cls_specific=bool(mc[2]), num_classes=mc[3], tile=tuple(mc[4:7]))
    if d["mode"] == "spot":
        d["spots"] = g[p + "spots"]
    else:
        d["markers"], d["volume"] = g[p + "markers"], g[p + "volume"]
    return d


_memo = {}


def sampled(g, name):
    """the box-head rows of a golden case (restatement), computed once and shared; callers must not change it"""
    if name not in _memo:
        d = case_inputs(g, name)
        _memo[name] = BR.box_head_targets(d["gt"], d["proposals"], d["box_cfg"], d["seed"], d["classes"], d["crowd"])
    return _memo[name]


def restated(g, name, form):
    key = (name, form)
    if key not in _memo:
        d, T = case_inputs(g, name), sampled(g, name)
        kw = dict(spots=d["spots"], in_size=d["tile"]) if d["mode"] == "spot" else dict(gt_boxes=d["gt"], markers=d["markers"],
                                                                                       label_volume=d["volume"])
        _memo[key] = MR.mask_targets(T["labels"], T["rois"], d["M"], form=form, classes=d["classes"], crowd=d["crowd"],
                                     num_classes=d["num_classes"], cls_specific=d["cls_specific"], **kw)
    return _memo[key]


def loss_inputs(seed, shape):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal(shape) * 3
    far = rng.rand(*shape) < 0.05
    return np.where(far, np.sign(x) * rng.uniform(20, 60, shape), x).astype(f32)


def loss_case(g, lname):
    """logits [rows, Cm, M, M, M], targets int32 [rows, Cm M^3], weight"""
    name = LOSS_CASES[lname]
    rows, M = int(g[lname + "_rows"]), int(g[name + "_mask_cfg"][0])
    t = g[name + "_masks"][:rows].astype(np.int32)
    Cm = t.shape[1] // M ** 3
    return loss_inputs(int(g[lname + "_seed"]), (rows, Cm, M, M, M)), t, float(g[lname + "_weight"])


def check_targets(T, g, name, what=""):
    """a trimmed target set (dict of masks, rois, assign, counts) against the reference's blobs, bit for bit"""
    p = name + "_"
    assert np.array_equal(np.asarray(T["counts"]), g[p + "counts"]), (what, T["counts"], g[p + "counts"])
    assert np.array_equal(np.asarray(T["masks"]), g[p + "masks"].astype(np.int32)), what
    assert np.asarray(T["masks"]).dtype == np.int32 and np.asarray(T["assign"]).dtype == np.int32
    assert np.array_equal(np.asarray(T["assign"]), g[p + "assign"]), what
    assert np.array_equal(np.ascontiguousarray(T["rois"], f32).view(np.uint32), g[p + "rois"].view(np.uint32)), what


@pytest.mark.parametrize("form", ["closed", "direct"])
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(g, name, form):
    check_targets(restated(g, name, form), g, name, form)


def test_fixture_holds_the_cases_it_claims(g):
    M = 14
    s = g["spot_small_rois"]
    e = s[:, 3:] - s[:, :3]
    assert (e < 2).any() and (e == 14).any() and (e == 15).any() and (e >= 29).any()
    b = g["spot_big_rois"]
    assert (b[:, 3:] - b[:, :3] >= 60).any() and tuple(g["spot_big_mask_cfg"][4:7]) == (64, 256, 256)
    m = g["spot_small_masks"].astype(np.int32)
    per = m.sum(1)
    assert (per == 0).any() and (per == M ** 3).any() and ((per > 0) & (per < M ** 3)).any()
    sp, a = g["spot_small_spots"], g["spot_small_assign"]
    assert ((sp[a, 0] < s[:, 0]) & (per > 0)).any()                                   # a centre outside its RoI, mask not empty
    T = sampled(g, "spot_small")
    L = BR.label(g["spot_small_gt"], g["spot_small_proposals"], g["spot_small_gt_classes"], g["spot_small_gt_crowd"])
    assert (L["assign"][T["rows"][:len(a)]] != a).any()                               # spot-box arg-max != box-head assignment
    boxes = MR.spots_to_boxes(sp, (32, 64, 48))
    el = MR.eligible(len(sp), g["spot_small_gt_classes"], g["spot_small_gt_crowd"])
    from rpn_train_reference import overlaps
    assert (overlaps(s, boxes[el]).max(1) == 0).any()                                 # an all-zero-IoU row
    assert g["spot_small_gt_crowd"].any() and not np.isin(np.flatnonzero(g["spot_small_gt_crowd"]), a).any()
    c3 = g["spot_3cls_masks"].reshape(-1, 3, M ** 3)
    lab = g["spot_3cls_labels"][:len(c3)]
    assert int(g["spot_3cls_mask_cfg"][2]) == 1 and set(lab.tolist()) == {1, 2} and (g["spot_3cls_gt_classes"] > 0).all()
    for i, l in enumerate(lab):
        assert (np.delete(c3[i], l, 0) == -1).all() and (c3[i, l] > -1).all()
    v, mr = g["mask_small_volume"], g["mask_small_rois"]
    assert ((v[:, :, 20] == 3) & (v[:, :, 21] == 4)).any() and v.dtype == np.uint16 and g["mask_small_markers"].max() > 255
    ti = MR.trunc_box(mr)
    assert (ti[:, 3:] == ti[:, :3]).any() and (g["mask_small_gt"][:, 3:] == np.array([47, 63, 31])).all(1).any()
    assert g["spot_nofg_counts"][0] == 0 and g["mask_nofg_counts"][0] == 0 and g["spot_small_counts"][0] > 0
    for lname in LOSS_CASES:
        x, t, _ = loss_case(g, lname)
        assert (x > 0).any() and (x < 0).any() and (np.abs(x) > 20).any() and (t > -1).any()
    assert os.path.getsize(GOLD) < 1000000 and g["spot_small_masks"].dtype == np.int8


def interval_rows(n, M):
    """the impulse definition as (lo, hi) per output index; asserts that every row is a non-empty interval"""
    F = MR.impulse_table(n, M)
    lo, hi = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for i in range(M):
        idx = np.flatnonzero(F[i])
        assert len(idx) and idx[-1] - idx[0] + 1 == len(idx), (n, M, i)
        lo[i], hi[i] = idx[0], idx[-1]
    return lo, hi


@pytest.mark.parametrize("M,top", [(14, 256), (7, 64), (28, 64)])
def test_interval_tables_equal_the_impulse_definition(M, top):
    """What the kernel's footprint() rests on, in one dimension: for every source length the closed-form ends are exactly the set of unit
    impulses that give resize > 0 at that output index.  (The 3-D predicate is the next two tests.)"""
    widths = {}
    for n in range(2, top + 1):
        want, got = interval_rows(n, M), MR.interval_table(n, M)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, M)
        widths[n] = int((want[1] - want[0]).max()) + 1
    if M == 14:
        assert widths[14] == 1 and widths[15] == 2 and all(widths[n] == 2 for n in range(2, 14)) and widths[28] == 6 and widths[60] == 16
        assert widths[255] == 70
        for n in (257, 258, 450, 511, 777, 1023, 1024):          # a sample up to the device's clamp; 258 and 450 have a tiny corner
            want, got = interval_rows(n, M), MR.interval_table(n, M)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (n, M)


def affected_lengths(M, top):
    return [n for n in range(2, top + 1) if MR.tiny_corners(n, M)]


def test_lengths_where_the_reference_underflows():
    """The lengths at M = 14 whose fp64 coordinate lands a few 1e-15 beside an integer, and the smallest counter-example to
    "closed form == reference": one voxel of an 18^3 volume.  The upper corner of output index 10 has weight 1.8e-15; alone it counts
    (the 1-D footprint holds it), times the Gaussian tails of the other two axes (2.3e-11 each) the reference's fp32 result is 0."""
    aff = affected_lengths(14, 1024)
    assert aff[:8] == [18, 34, 58, 82, 122, 130, 150, 158] and len(aff) == 42 and sum(len(MR.tiny_corners(n, 14)) for n in aff) == 60
    assert MR.tiny_corners(18, 14) == [10] and not any(MR.tiny_corners(n, 14) for n in (14, 15, 16, 17, 19, 28, 60))
    v = np.zeros((18, 18, 18), f32)
    v[15, 15, 15] = 1
    ref, wide = MR.resize_positive(v, 14), MR.resize_positive(v, 14, fp64=True)
    closed = v > 0
    for axis in (2, 1, 0):
        closed = MR.interval_any(closed, axis, *MR.table(18, 14))
    assert np.array_equal(closed, wide) and (closed | ~ref).all()
    assert int(closed.sum()) == 64 and int(ref.sum()) == 51                          # 13 voxels the reference underflows
    extra = np.argwhere(closed & ~ref)
    assert (extra == 10).any(1).all()                                                 # all of them on the tiny corner's output index


def spot_case(rng, ext):
    lo = rng.uniform(0, 40, 3)
    box = np.concatenate([lo, lo + ext]).astype(f32)
    ctr = lo + ext * rng.uniform(-0.3, 1.3, 3)
    r = rng.choice([0.4, 1.0, 2.5, 6, 15, 30]) * rng.uniform(0.8, 1.2)
    return np.array([ctr[0], ctr[1], ctr[2], r], f32), box


def label_case(rng, k, ext):
    """a sparse label volume around an RoI of the given extents and an object box a few voxels off it"""
    dims = (np.ceil(ext[::-1]) + rng.randint(4, 12, 3)).astype(int)
    lab = ((rng.rand(*dims) < rng.choice([0.002, 0.02, 0.2])) * 7).astype(np.uint16 if k % 2 else np.int32)
    lo = rng.uniform(-3, 3, 3)
    box = np.concatenate([lo, lo + ext]).astype(f32)
    gt = np.concatenate([lo + rng.uniform(-4, 4, 3), lo + ext + rng.uniform(-4, 4, 3)]).astype(f32)
    return lab, gt, box


def compare_forms(closed, ref, wide, extents, M=14):
    """closed == the fp64 evaluation; closed contains the reference; they differ only on an output index with a tiny corner.
    -> number of voxels the reference underflows"""
    assert np.array_equal(closed, wide)
    assert not (ref & ~closed).any()
    extra = np.argwhere(closed & ~ref)
    tiny = [set(MR.tiny_corners(e, M)) for e in extents]
    assert all(any(int(v[a]) in tiny[a] for a in range(3)) for v in extra), (extents, extra[:4])
    return len(extra)


def test_closed_form_against_both_resizes_on_random_inputs():
    """240 spheres and 48 label volumes with extents drawn uniformly, then 240 + 60 with every extent on a length that has a tiny corner
    (18, 34, 58): the closed form is the fp64 evaluation of resize > 0 everywhere; it equals the reference's fp32 result whenever no
    axis has a tiny corner, contains it always, and where they differ the voxel lies on a tiny corner's output index."""
    rng = np.random.RandomState(1)
    nonempty = full = 0
    for k in range(240):
        spot, box = spot_case(rng, rng.uniform(1, 60, 3) if k % 3 else rng.uniform(1, 6, 3))
        ext = MR.spot_geometry(spot, box)[0]
        ref = MR.spot_mask_direct(spot, box, 14) > 0
        n = compare_forms(MR.spot_mask_closed(spot, box, 14) > 0, ref, MR.spot_mask_direct(spot, box, 14, fp64=True) > 0, ext)
        assert n == 0 or any(MR.tiny_corners(e, 14) for e in ext)
        nonempty += int(ref.any())
        full += int(ref.all())
    assert nonempty > 100 and full > 20
    nonempty = 0
    for k in range(48):
        lab, gt, box = label_case(rng, k, rng.uniform(0, 50, 3))
        ext = MR.label_region(gt, box, lab.shape)[0]
        ref = MR.label_mask_direct(lab, 7, gt, box, 14) > 0
        n = compare_forms(MR.label_mask_closed(lab, 7, gt, box, 14) > 0, ref, MR.label_mask_direct(lab, 7, gt, box, 14, fp64=True) > 0, ext)
        assert n == 0 or any(MR.tiny_corners(e, 14) for e in ext)
        nonempty += int(ref.any())
    assert nonempty > 20
    # aimed at the affected lengths, on all three axes
    masks = voxels = 0
    for k in range(240):
        spot, box = spot_case(rng, rng.choice([18, 34, 58], 3) + rng.uniform(0.01, 0.99, 3))
        ext = MR.spot_geometry(spot, box)[0]
        assert all(e in (18, 34, 58) for e in ext)
        n = compare_forms(MR.spot_mask_closed(spot, box, 14) > 0, MR.spot_mask_direct(spot, box, 14) > 0,
                          MR.spot_mask_direct(spot, box, 14, fp64=True) > 0, ext)
        masks, voxels = masks + (n > 0), voxels + n
    print("spheres on affected extents: %d of 240 masks differ from the reference, %d voxels" % (masks, voxels))
    assert masks > 0                                                                  # the difference is real: DESIGN documents it
    masks = voxels = 0
    for k in range(60):
        lab, gt, box = label_case(rng, k, rng.choice([18, 34], 3) + rng.uniform(0.01, 0.99, 3))
        ext = MR.label_region(gt, box, lab.shape)[0]
        n = compare_forms(MR.label_mask_closed(lab, 7, gt, box, 14) > 0, MR.label_mask_direct(lab, 7, gt, box, 14) > 0,
                          MR.label_mask_direct(lab, 7, gt, box, 14, fp64=True) > 0, ext)
        masks, voxels = masks + (n > 0), voxels + n
    print("label volumes on affected extents: %d of 60 masks differ from the reference, %d voxels" % (masks, voxels))
    assert masks > 0


@pytest.mark.parametrize("lname", sorted(LOSS_CASES))
def test_reference_loss_lies_within_bounds_of_the_restatement(g, lname):
    x, t, weight = loss_case(g, lname)
    l64, g64, W, abs_sum = MR.loss(x, t, weight)
    _, ref_loss, _, ref_grad = MR.loss_bounds(l64, g64, W, abs_sum, weight, x.size)
    got, gg = float(g[lname + "_loss"]), g[lname + "_grad"].astype(np.float64)
    print(lname, "reference loss err", abs(got - l64), "of", ref_loss, "| grad err", np.abs(gg - g64).max(), "of", ref_grad.min())
    assert abs(got - l64) <= ref_loss
    assert (np.abs(gg - g64) <= ref_grad).all() and not gg.reshape(t.shape)[t == -1].any() and not g64.reshape(t.shape)[t == -1].any()
    l0, g0, W0, _ = MR.loss(x, np.full_like(t, -1), weight)
    assert l0 == 0 and W0 == 0 and not g0.any()                                       # defined where the reference divides 0 by 0


@pytest.mark.ref
def test_live_generator_equals_committed_file(g):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD)))
    import ref_harness
    if not ref_harness.available():
        pytest.skip("reference tree not present")
    import gen_mask_train
    live = gen_mask_train.build_arrays()
    assert sorted(live) == sorted(g)
    for k in g:
        a, b = np.asarray(live[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def test_argument_validation_without_gpu():
    """Both entry points reject bad arguments and the documented limits before they follow a pointer or launch anything."""
    import __graft_entry__ as entry
    entry.build()
    from m3d._lib import LIB_PATH, MaskImage
    L = ctypes.CDLL(LIB_PATH)
    L.m3d_mask_loss_workspace_bytes.restype = ctypes.c_size_t
    one, odd = ctypes.c_void_p(256), ctypes.c_void_p(258)      # never dereferenced: every call below fails validation first
    off = (ctypes.c_int32 * 3)(0, 4, 6)
    size = (ctypes.c_int32 * 3)(32, 64, 48)

    def image(ptr=256, dtype=0, dims=(32, 64, 48)):
        im = MaskImage()
        im.labels, im.dtype, (im.depth, im.height, im.width) = ptr, dtype, dims
        return im
    two = (MaskImage * 2)(image(), image(dtype=1))

    def targets(B=2, batch=64, fg=16, M=14, C=2, spec=0, mode=0, offp=off, labels=one, rois=one, counts=one, spots=one, sizep=size,
                gt=one, markers=one, images=two, masks=one, mrois=one, assign=one, mcounts=one, classes=None):
        return L.m3d_mask_targets(labels, rois, counts, B, batch, fg, M, C, spec, mode, offp, classes, None, spots, sizep, gt, markers, images,
                                  masks, mrois, assign, mcounts, None)
    inv, uns = -1, -4
    assert targets(B=0) == inv and targets(batch=0) == inv and targets(fg=0) == inv and targets(M=1) == inv and targets(C=1) == inv
    assert targets(mode=2) == inv and targets(mode=-1) == inv and targets(offp=None) == inv
    assert targets(offp=(ctypes.c_int32 * 3)(0, 4, 3)) == inv and targets(offp=(ctypes.c_int32 * 3)(1, 4, 6)) == inv
    for name in ("labels", "rois", "counts", "masks", "mrois", "assign", "mcounts"):
        assert targets(**{name: None}) == inv and targets(**{name: odd}) == inv, name
    assert targets(spots=None) == inv and targets(spots=odd) == inv and targets(sizep=None) == inv and targets(classes=odd) == inv
    assert targets(sizep=(ctypes.c_int32 * 3)(32, 0, 48)) == inv
    assert targets(mode=1, gt=None) == inv and targets(mode=1, markers=None) == inv and targets(mode=1, images=None) == inv
    assert targets(mode=1, gt=odd) == inv and targets(mode=1, markers=odd) == inv
    assert targets(mode=1, images=(MaskImage * 2)(image(), image(dtype=2))) == inv              # a label dtype other than the two
    assert targets(mode=1, images=(MaskImage * 2)(image(), image(ptr=0))) == inv                # objects but no volume
    assert targets(mode=1, images=(MaskImage * 2)(image(), image(ptr=258, dtype=1))) == inv     # a misaligned volume
    assert targets(mode=1, images=(MaskImage * 2)(image(), image(dims=(32, 0, 48)))) == inv
    assert targets(mode=1, offp=(ctypes.c_int32 * 3)(0, 6, 6)) == inv                           # mask mode: an image without objects
    assert targets(B=65) == uns and targets(M=33) == uns and targets(C=65) == uns and targets(fg=4097) == uns
    assert targets(offp=(ctypes.c_int32 * 3)(0, 2049, 2050)) == uns                             # K > 2048 in an image

    loss = L.m3d_mask_loss
    i64, dbl, sz = ctypes.c_int64, ctypes.c_double, ctypes.c_size_t

    def run(N=16, Cm=1, M=14, pred=one, masks=one, out=one, num=one, grad=one, ws=one, wsb=1 << 20):
        return loss(pred, masks, i64(N), Cm, M, dbl(1.0), out, num, grad, ws, sz(wsb), None)
    assert run(N=-1) == inv and run(Cm=0) == inv and run(M=1) == inv
    for name in ("pred", "masks", "out", "grad", "ws"):
        assert run(**{name: None}) == inv and run(**{name: odd}) == inv, name
    assert run(num=odd) == inv
    assert run(M=33) == uns and run(Cm=65) == uns and run(N=64 * 4096 + 1) == uns and run(N=64 * 4096, Cm=2, M=32) == uns
    assert run(wsb=0) == -3
    need = L.m3d_mask_loss_workspace_bytes
    assert need(i64(16), 1, 14) > 0 and need(i64(16), 1, 33) == 0 and need(i64(-1), 1, 14) == 0 and need(i64(64 * 4096), 2, 32) == 0
    assert need(i64(32), 1, 14) >= need(i64(16), 1, 14)


def test_config_and_head_names():
    import torch
    import m3d
    with pytest.raises(TypeError):
        m3d.MaskTrainCfg.nuclei(resolutoin=28)                 # a misspelt key is an error, not a silent default
    with pytest.raises(ValueError):
        m3d.MaskTrainCfg(anno_type="polygon")
    n, s = m3d.MaskTrainCfg.nuclei(), m3d.MaskTrainCfg.soma()
    assert (n.anno_type, n.num_convs, tuple(n.in_size)) == ("mask", 3, (64, 256, 256))
    assert (s.anno_type, s.num_convs, tuple(s.in_size)) == ("spot", 4, (64, 256, 256))
    for c in (n, s):
        assert (c.resolution, c.cls_specific, c.weight_loss_mask, c.num_classes) == (14, False, 1.0, 2)
        assert (c.roi_xform_resolution, c.sampling_ratio, c.dim_reduced, c.mask_classes) == (7, 2, 256, 1)
    assert m3d.MaskTrainCfg.soma(cls_specific=True, num_classes=3).mask_classes == 3
    cfg = m3d.MaskTrainCfg.soma(dim_reduced=8)
    head = m3d.MaskHead(4, cfg, stride=4)
    want = ["conv_fcn.%d.%s" % (2 * i, k) for i in range(4) for k in ("weight", "bias")] + ["upconv.weight", "upconv.bias",
                                                                                            "classify.weight", "classify.bias"]
    assert list(head.state_dict()) == want
    assert tuple(head.conv_fcn[0].weight.shape) == (8, 4, 3, 3, 3) and tuple(head.upconv.weight.shape) == (8, 8, 2, 2, 2)
    assert tuple(head.classify.weight.shape) == (1, 8, 1, 1, 1) and head.spatial_scale == 0.25
    # mask_rcnn_heads.py:38-46: the classifier is MSRAFill (std sqrt(2 / fan_out)) with class-specific masks, normal(0.001) without
    assert 0.0005 < float(head.classify.weight.detach().std()) < 0.002
    spec = m3d.MaskHead(4, m3d.MaskTrainCfg.soma(cls_specific=True, num_classes=3, dim_reduced=128), stride=4)
    assert tuple(spec.classify.weight.shape) == (3, 128, 1, 1, 1) and abs(float(spec.classify.weight.detach().std()) / (2.0 / 3) ** 0.5 - 1) < 0.2
    from m3d.train import _per_image
    with pytest.raises(m3d.M3DError, match="^mask_targets: gt_classes has 2 entries for 3 boxes"):
        _per_image([np.ones(2, np.int32)], [torch.zeros((3, 6))], torch.int32, "cpu", "gt_classes", "mask_targets")
    with pytest.raises(m3d.M3DError, match="^box_head_targets: gt_crowd"):
        _per_image([np.ones(2, np.int32)], [torch.zeros((3, 6))], torch.uint8, "cpu", "gt_crowd")
    ds = head.detector_state()
    assert sorted(ds) == sorted(["Mask_Head." + k for k in want[:-2]] + ["Mask_Outs." + k for k in want[-2:]])
    other = m3d.MaskHead(4, cfg, stride=4)
    other.load_detector_state(ds)
    assert all(torch.equal(a, b) for a, b in zip(head.state_dict().values(), other.state_dict().values()))
    # no CPU path
    T = m3d.BoxHeadTargets(torch.zeros((1, 64), dtype=torch.int64), torch.zeros((1, 64), dtype=torch.int32), torch.zeros((1, 64, 6)),
                           torch.zeros((1, 64, 6)), torch.zeros((1, 8), dtype=torch.int64), m3d.BoxHeadTrainCfg.nuclei())
    with pytest.raises(m3d.M3DError):
        m3d.mask_targets(T, s, spots=[np.zeros((1, 4), f32)])
    MT = m3d.MaskTargets(torch.full((1, 16, 2744), -1, dtype=torch.int32), torch.zeros((1, 16, 6)), torch.zeros((1, 16), dtype=torch.int32),
                         torch.zeros((1, 4), dtype=torch.int64), T.labels, s)
    with pytest.raises(m3d.M3DError):
        m3d.mask_losses(torch.zeros((16, 1, 14, 14, 14)), MT)
    with pytest.raises(NotImplementedError):
        head(torch.zeros((1, 4, 4, 8, 8)), torch.zeros((2, 7)))


def test_gt_spots_follow_the_crop():
    """Batch.gt_spots against blob.py:153-161: the kept spheres move by the crop origin and are clipped to the tile, radius untouched."""
    import torch
    from m3d.data import Batch, SampleCfg
    cfg = SampleCfg.soma()
    S, H, W = cfg.IN_SIZE
    rng = np.random.RandomState(3)
    segms = [np.concatenate([rng.uniform(0, 400, (6, 3)), rng.uniform(2, 20, (6, 1))], 1).astype(f32) for _ in range(2)]
    keep = np.array([[0, 2, 3, 5, -1, -1], [1, 4, -1, -1, -1, -1]], np.int32)
    info = np.array([[37, 120, 9, 4, 0, 12, 0, 0], [0, 0, 0, 2, 0, 1, 0, 0]], np.int32)
    dataset = types.SimpleNamespace(classes=[np.ones(6, np.int32)] * 2, crowd=[np.zeros(6, bool)] * 2, segms=segms, cfg=cfg)
    host = torch.from_numpy(np.concatenate([info.reshape(-1), keep.reshape(-1)]))
    event = types.SimpleNamespace(synchronize=lambda: None)
    batch = Batch(dataset, [0, 1], None, torch.zeros((2, 6, 6)), None, None, None, host, event)
    got = batch.gt_spots
    for b in range(2):
        n = info[b, 3]
        sp = segms[b][keep[b, :n]].copy()                       # blob.py:104, 153-161 on the kept rows
        x, y, z = (int(v) for v in info[b, :3])
        sp[:, 0] -= x
        sp[:, 1] -= y
        sp[:, 2] -= z
        np.clip(sp[:, 0], 0, W - 1, out=sp[:, 0])
        np.clip(sp[:, 1], 0, H - 1, out=sp[:, 1])
        np.clip(sp[:, 2], 0, S - 1, out=sp[:, 2])
        assert got[b].dtype == f32 and np.array_equal(got[b], sp) and np.array_equal(got[b][:, 3], segms[b][keep[b, :n], 3])
        assert len(batch.gt_boxes[b]) == n
    assert (got[0][:, :3] == 0).any() or (got[0][:, 0] == W - 1).any()          # the clip bites in this sample
    dataset.segms = [None, None]
    assert Batch(dataset, [0, 1], None, torch.zeros((2, 6, 6)), None, None, None, host, event).gt_spots == [None, None]
