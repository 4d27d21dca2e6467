"""CPU: the NumPy restatement of the reference's evaluation scripts (tests/eval_reference.py) reproduces the reference's own results
(tests/golden/eval.npz, made by gen_eval.py), and the host parts of m3d.evaluate - voc_ap, greedy assignment, the tie rule,
load_gt_bbox, slice normalisation, the detection F1 and the edge cases - match it."""
import os

import numpy as np
import pytest

import eval_reference as R
from m3d import evaluate as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval.npz")
TAGS = {0.3: "03", 0.5: "05", 0.7: "07"}


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def images(g):
    n = len([k for k in g if k.startswith("gt_") and not k.startswith("gt_bbox")])
    return [(g["gt_%d" % k], g["pred_%d" % k], g["table_%d" % k]) for k in range(n)]


def gt_boxes(g, k):
    b = g["gt_bbox_%d" % k]
    return np.stack([b[:, 1], b[:, 2], b[:, 3], b[:, 1] + b[:, 4] - 1, b[:, 2] + b[:, 5] - 1, b[:, 3] + b[:, 6] - 1], 1).astype(np.float32)


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("t", sorted(TAGS))
def test_restatement_soma_matches_reference(g, t):
    imgs = images(g)
    prec, rec, ap, per = R.soma([p for _, p, _ in imgs], [gt for gt, _, _ in imgs], [tb for _, _, tb in imgs], t)
    tag = TAGS[t]
    assert np.array_equal(bits(prec), bits(g["soma_prec_" + tag]))
    assert np.array_equal(bits(rec), bits(g["soma_rec_" + tag]))
    assert bits(ap) == bits(g["soma_ap_" + tag])
    with_preds = [v for v, (_, _, tb) in zip(per, imgs) if len(tb)]      # the reference prints an AP only for images with predictions
    assert np.array_equal(bits(with_preds), bits(g["soma_per_image_ap_" + tag]))


def test_restatement_iou_matches_mask_iou_fast(g):
    gt, pred, _ = images(g)[0]
    iou = R.iou_matrix(pred, gt, g["iou0_rows"], g["iou0_cols"])
    assert iou.dtype == np.float32 and np.array_equal(iou.view(np.uint32), g["iou0"].view(np.uint32))
    # the fixture holds the edge cases it claims: an absent id (zero row), a tie, an IoU of exactly float32(0.7)
    assert (iou == 0).all(axis=1).any()
    assert (iou == np.float32(0.7)).any()
    assert any(np.sum(r == r.max()) > 1 and r.max() > 0 for r in iou)


def test_restatement_nuclei_matches_reference(g):
    n = len(images(g))
    dets7 = [g["det_rows_%d" % k][:, 1:].astype(np.float32) for k in range(n)]
    f1, p, r, tp, fp = R.detection(dets7, [gt_boxes(g, k) for k in range(n)])
    assert bits(f1) == bits(g["det_f1score_det"]) and bits(p) == bits(g["det_precision_det"]) and bits(r) == bits(g["det_recall_det"])
    assert np.array_equal(tp, g["det_tp"]) and np.array_equal(fp, g["det_fp"])
    imgs = images(g)
    f1, p, r, tpp, gtp, prp = R.segmentation([pr for _, pr, _ in imgs], [gt for gt, _, _ in imgs],
                                             [g["det_rows_%d" % k][:, 1:7].astype(float) for k in range(n)], [gt_boxes(g, k) for k in range(n)])
    assert (tpp, gtp, prp) == (g["seg_tp_pixel"], g["seg_gt_pixel"], g["seg_pre_pixel"])
    assert bits(p) == bits(g["seg_precision"]) and bits(r) == bits(g["seg_recall"]) and bits(f1) == bits(g["seg_f1score_det"])


def test_detection_f1_host_matches_reference(g):
    n = len(images(g))
    r = E.detection_f1([g["det_rows_%d" % k][:, 1:].astype(np.float32) for k in range(n)], [gt_boxes(g, k) for k in range(n)])
    assert bits(r["f1"]) == bits(g["det_f1score_det"]) and bits(r["precision"]) == bits(g["det_precision_det"])
    assert bits(r["recall"]) == bits(g["det_recall_det"])
    assert np.array_equal(r["tp"], g["det_tp"]) and np.array_equal(r["fp"], g["det_fp"])
    # the score at exactly float32(0.4) is dropped by the fp32 comparison; in fp64 it would have been kept
    s = np.float32(0.4)
    assert not (s > 0.4) and float(s) > 0.4
    assert len(r["tp"]) == sum(int(np.sum(g["det_rows_%d" % k][:, 7].astype(np.float32) > 0.4)) for k in range(n))


def test_voc_ap_bits():
    rng = np.random.RandomState(0)
    for n in (1, 2, 7, 100, 1000):
        m = (rng.uniform(size=n) < 0.6).astype(np.int8)
        tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
        prec, rec = tp / (fp + tp), tp / max(1, rng.randint(1, n + 5))
        assert bits(E.voc_ap(rec, prec)[2]) == bits(R.voc_ap(rec, prec))
    with pytest.raises(NotImplementedError):
        E.voc_ap(np.ones(3), np.ones(3), use_07_metric=True)
    with pytest.raises(NotImplementedError):
        E.eval_instance_segmentation_soma("/nonexistent", "/nonexistent", ["x"], 0.5, use_07_metric=True)


def test_assign_matches_threshold_and_greedy():
    t = 0.7
    assert E.assign_matches(np.array([np.float32(0.7)], np.float32), np.array([0]), t, 1) == [1]        # equal in fp32: a match
    assert E.assign_matches(np.array([np.nextafter(np.float32(0.7), np.float32(0))], np.float32), np.array([0]), t, 1) == [0]
    # rows in score order: the second row on GT 1 is a FP and does not fall back to another GT; -1 rows are FPs
    assert E.assign_matches(np.array([0.9, 0.8, 0.2, 0.95], np.float32), np.array([1, 1, 0, 0]), 0.5, 3) == [1, 0, 0, 1]


def test_score_order_ties_descending_index():
    s = np.array([0.5, 0.9, 0.5, 0.1, 0.9])
    assert list(E.score_order(s)) == [4, 1, 2, 0, 3]


def test_pool_prec_rec_and_edge_cases():
    with pytest.raises(ValueError):
        E.pool_prec_rec([0.5], [0], 0)
    prec, rec = E.pool_prec_rec([0.2, 0.9, 0.5], [1, 1, 0], 4)
    assert list(prec) == [1.0, 0.5, 2 / 3] and list(rec) == [0.25, 0.25, 0.5]
    with pytest.raises(ValueError):
        E._table(np.array([[0, 0.5], [3, 0.2]]))
    t, ids = E._table(np.array([[3, 0.2], [5, 0.7], [4, 0.2]]))
    assert list(ids) == [5, 4, 3]
    r = E.detection_f1([np.zeros((0, 7), np.float32)], [np.zeros((2, 6), np.float32)])
    assert np.isnan(r["f1"]) and np.isnan(r["precision"]) and r["recall"] == 0


def test_load_gt_bbox(tmp_path, g):
    b = g["gt_bbox_2"]
    p = tmp_path / "bbox_002.txt"
    p.write_text("header line\n" + "".join(" ".join(str(int(v)) for v in r) + "\n" for r in b))
    boxes, markers = E.load_gt_bbox(str(p))
    assert boxes.dtype == np.float32 and np.array_equal(boxes, gt_boxes(g, 2))
    assert markers.dtype == np.int64 and np.array_equal(markers, b[:, 7])
    e = tmp_path / "empty.txt"
    e.write_text("header\n")
    boxes, markers = E.load_gt_bbox(str(e))
    assert boxes.shape == (0, 6) and markers.dtype == np.uint16


def test_box_slices_follow_numpy_slicing():
    rng = np.random.RandomState(3)
    shape = (6, 9, 11)
    vol = np.arange(np.prod(shape)).reshape(shape)
    for _ in range(500):
        bb = rng.uniform(-14, 16, 6)
        x1, y1, z1, x2, y2, z2 = bb.astype(int)
        want = vol[z1:z2 + 1, y1:y2 + 1, x1:x2 + 1]
        z0, z1_, y0, y1_, x0, x1_ = E.box_slices(bb, shape)
        assert 0 <= z0 <= z1_ <= shape[0] and 0 <= y0 <= y1_ <= shape[1] and 0 <= x0 <= x1_ <= shape[2]
        assert np.array_equal(vol[z0:z1_, y0:y1_, x0:x1_], want)
