"""GPU: the label-volume evaluation path (csrc/eval3d.hip, m3d.evaluate, tools/evaluate.py) against a NumPy contingency table, the
NumPy restatement of the reference scripts (tests/eval_reference.py) and the reference's own results (tests/golden/eval.npz)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_reference as R
import m3d
from m3d import evaluate as E
from m3d.io import save_segmentation, write_tiff_stack, save_detections
from m3d.synth import synth_label_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval.npz")
TAGS = {0.3: "03", 0.5: "05", 0.7: "07"}


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def check_overlap(a, b, **kw):
    ov = m3d.label_overlap(a, b, **kw)
    ca, cb, pairs, cnt = R.contingency(a, b)
    ga, gb = ov.count_a.cpu().numpy(), ov.count_b.cpu().numpy()
    assert np.array_equal(ga[:len(ca)], ca) and not ga[len(ca):].any()
    assert np.array_equal(gb[:len(cb)], cb) and not gb[len(cb):].any()
    assert np.array_equal(ov.pairs.cpu().numpy(), pairs) and np.array_equal(ov.counts.cpu().numpy(), cnt)
    return ov


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_label_overlap_against_contingency(dtype):
    rng = np.random.RandomState(0)
    gt, pred, _ = synth_label_pair((7, 33, 65), 12, 5)
    check_overlap(pred.astype(dtype), gt.astype(dtype))
    z = np.zeros((7, 33, 65), dtype)
    check_overlap(z, z)                                               # all background
    one = z.copy()
    one[3, 17, 40] = 5
    check_overlap(one, one[::-1].copy())
    check_overlap(one, one)                                           # a single voxel
    a = rng.randint(0, 300, (5, 31, 67)).astype(dtype)                # every voxel a random pair: ~V distinct pairs
    b = rng.randint(0, 300, (5, 31, 67)).astype(dtype)
    check_overlap(a, b, max_a=299, max_b=299)
    t = torch.from_numpy(a).cuda()
    check_overlap(a, b)                                               # NumPy and CUDA inputs alike
    assert m3d.label_overlap(t, torch.from_numpy(b).cuda()).pairs.shape[0] == R.contingency(a, b)[2].shape[0]


def test_label_overlap_extreme_ids():
    a = np.zeros((3, 5, 70), np.uint16)
    b = np.zeros_like(a)
    a[1, 2, 10:30] = 65535
    b[1, 2, 20:40] = 65535
    b[0, 0, :5] = 1
    check_overlap(a, b)
    big = (1 << 24) - 1
    ai, bi = a.astype(np.int32), b.astype(np.int32)
    ai[2, 4, 60:] = big
    bi[2, 4, 65:] = big - 3
    ov = check_overlap(ai, bi)
    assert ov.count_a.numel() == big + 1
    with pytest.raises(m3d.M3DError):
        m3d.label_overlap(ai, bi, max_a=1000)                          # a label above the declared maximum
    with pytest.raises(m3d.M3DError):
        m3d.label_overlap(ai + (1 << 24) * (ai > 0), bi)               # >= 2^24


def test_label_overlap_relaunch_and_determinism():
    rng = np.random.RandomState(1)
    a = rng.randint(0, 2000, (9, 40, 77)).astype(np.int32)
    b = rng.randint(0, 2000, (9, 40, 77)).astype(np.int32)
    small = check_overlap(a, b, capacity=16)                          # table full -> one re-launch at the proven bound
    again = m3d.label_overlap(a, b)
    assert np.array_equal(small.pairs.cpu().numpy(), again.pairs.cpu().numpy())
    assert np.array_equal(small.counts.cpu().numpy(), again.counts.cpu().numpy())
    gt, pred, _ = synth_label_pair((32, 96, 96), 60, 2)
    r1, r2 = m3d.label_overlap(pred, gt), m3d.label_overlap(pred, gt)
    for x, y in zip(r1, r2):
        assert torch.equal(x, y)


def test_label_iou_bit_exact(tmp_path):
    g = np.load(GOLD)
    iou = E.label_iou(g["pred_0"], g["gt_0"], g["iou0_rows"], g["iou0_cols"])
    assert np.array_equal(iou.view(np.uint32), g["iou0"].view(np.uint32))
    gt, pred, table = synth_label_pair((16, 48, 48), 20, 3)
    rows = np.concatenate([table[:, 0].astype(np.int64), [pred.max() + 3]])            # an absent id
    gids = np.unique(gt)[1:]
    want = R.iou_matrix(pred, gt, rows, gids)
    got = E.label_iou(pred, gt, rows)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and not got[-1].any()
    best = m3d.label_iou_best(m3d.label_overlap(pred, gt), rows)
    mx, am = best.max_iou.cpu().numpy(), best.argmax.cpu().numpy()
    assert np.array_equal(mx.view(np.uint32), want.max(1).view(np.uint32)) and np.array_equal(am, want.argmax(1))


def test_soma_ap_against_reference():
    g = np.load(GOLD)
    n = 4
    for t, tag in TAGS.items():
        prec, rec, per = E.soma_prec_rec([g["pred_%d" % k] for k in range(n)], [g["gt_%d" % k] for k in range(n)],
                                         [g["table_%d" % k] for k in range(n)], t)
        assert np.array_equal(bits(prec), bits(g["soma_prec_" + tag])) and np.array_equal(bits(rec), bits(g["soma_rec_" + tag]))
        assert bits(E.voc_ap(rec, prec)[2]) == bits(g["soma_ap_" + tag])
        assert np.array_equal(bits([v for v in per if not np.isnan(v)]), bits(g["soma_per_image_ap_" + tag]))


def test_nuclei_segmentation_f1_against_reference():
    g = np.load(GOLD)
    n = 4
    gtb = []
    for k in range(n):
        b = g["gt_bbox_%d" % k]
        gtb.append(np.stack([b[:, 1], b[:, 2], b[:, 3], b[:, 1] + b[:, 4] - 1, b[:, 2] + b[:, 5] - 1, b[:, 3] + b[:, 6] - 1], 1).astype(np.float32))
    r = E.segmentation_f1([g["pred_%d" % k] for k in range(n)], [g["gt_%d" % k] for k in range(n)],
                          [g["det_rows_%d" % k][:, 1:7].astype(float) for k in range(n)], gtb)
    assert (r["tp_pixel"], r["gt_pixel"], r["pre_pixel"]) == (g["seg_tp_pixel"], g["seg_gt_pixel"], g["seg_pre_pixel"])
    assert bits(r["f1"]) == bits(g["seg_f1score_det"]) and bits(r["precision"]) == bits(g["seg_precision"])
    assert bits(r["recall"]) == bits(g["seg_recall"])


def test_box_union_counts_against_numpy():
    rng = np.random.RandomState(4)
    gt, pred, _ = synth_label_pair((13, 37, 71), 15, 6)
    for dt in (np.uint16, np.int32):
        boxes = rng.uniform(-20, 80, (40, 6))
        ranges = np.array([E.box_slices(b, gt.shape) for b in boxes])
        keep = np.zeros(gt.shape, bool)
        for z0, z1, y0, y1, x0, x1 in ranges:
            keep[z0:z1, y0:y1, x0:x1] = True
        want = [np.sum(pred > 0), np.sum(gt > 0), np.sum(keep & (pred > 0) & (gt > 0))]
        assert list(m3d.box_union_overlap_counts(pred.astype(dt), gt.astype(dt), ranges)) == want
    assert list(m3d.box_union_overlap_counts(pred, gt, np.zeros((0, 6)))) == [np.sum(pred > 0), np.sum(gt > 0), 0]


def test_known_answers():
    gt, _, _ = synth_label_pair((24, 64, 64), 30, 7)
    ids = np.unique(gt)[1:]
    if len(ids) % 2:                                                   # an even number of GT instances: half of them is exact
        gt[gt == ids[-1]] = 0
        ids = ids[:-1]
    perm = np.zeros(int(gt.max()) + 1, np.uint16)
    perm[ids] = np.random.RandomState(0).permutation(len(ids)) + 1
    pred = perm[gt]
    table = np.stack([np.arange(1, len(ids) + 1), np.linspace(0.9, 0.1, len(ids))], 1)
    prec, rec, _ = E.soma_prec_rec([pred], [gt], [table], 0.5)
    assert E.voc_ap(rec, prec)[2] == 1.0
    half = np.where(np.isin(gt, ids[::2]), gt, 0)                      # every other instance removed
    prec, rec, _ = E.soma_prec_rec([half], [gt], [np.stack([ids[::2], np.linspace(0.9, 0.1, len(ids[::2]))], 1)], 0.5)
    assert E.voc_ap(rec, prec)[2] == 0.5
    shifted = np.zeros_like(gt)
    shifted[:, :, 8:] = gt[:, :, :-8]                                  # far below any threshold
    prec, rec, _ = E.soma_prec_rec([shifted], [gt], [np.stack([ids, np.linspace(0.9, 0.1, len(ids))], 1)], 0.9)
    assert E.voc_ap(rec, prec)[2] == 0.0


def test_soma_edge_cases():
    gt, pred, table = synth_label_pair((8, 32, 32), 6, 8)
    empty = np.zeros_like(gt)
    with pytest.raises(ValueError):
        E.soma_prec_rec([pred], [empty], [table], 0.5)                 # no GT in any image
    prec, rec, per = E.soma_prec_rec([pred, pred], [empty, gt], [table, table], 0.5)
    assert np.isnan(per[0]) and not np.isnan(per[1])
    p2, r2, _ = E.soma_prec_rec([pred], [gt], [table], 0.5)
    assert len(prec) == 2 * len(table) and rec[-1] == r2[-1]           # the GT-less image's rows add FPs only
    bad = table.copy()
    bad[0, 0] = 0
    with pytest.raises(ValueError):
        E.soma_prec_rec([pred], [gt], [bad], 0.5)


@pytest.mark.parametrize("shape,n", [((96, 256, 256), 2500), ((59, 350, 350), 150)])
def test_full_size(shape, n):
    gt, pred, table = synth_label_pair(shape, n, 11)
    check_overlap(pred, gt)
    prec, rec, _ = E.soma_prec_rec([pred], [gt], [table], 0.5)
    p2, r2, ap2, _ = R.soma([pred], [gt], [table], 0.5)
    assert np.array_equal(bits(prec), bits(p2)) and np.array_equal(bits(rec), bits(r2))
    assert bits(E.voc_ap(rec, prec)[2]) == bits(ap2)


def test_files_end_to_end(tmp_path):
    imgs = [synth_label_pair((10, 40, 48), 8, 20 + k) for k in range(3)]
    # soma layout
    for k, (gt, pred, table) in enumerate(imgs):
        save_segmentation(str(tmp_path / "pred"), "i%d" % k, pred, table)
        os.makedirs(tmp_path / "gt" / ("i%d" % k))
        write_tiff_stack(str(tmp_path / "gt" / ("i%d" % k) / ("i%d.tif" % k)), gt)
    names = ["i%d" % k for k in range(3)]
    res = E.eval_instance_segmentation_soma(str(tmp_path / "pred"), str(tmp_path / "gt"), names, 0.5)
    prec, rec, per = E.soma_prec_rec([p for _, p, _ in imgs], [g for g, _, _ in imgs], [t for _, _, t in imgs], 0.5)
    assert res["ap"] == E.voc_ap(rec, prec)[2] and res["map"] == res["ap"] and res["per_image_ap"] == per
    # nuclei layout
    src = tmp_path / "ctc"
    for d in ("dets", "seg", "ctc/02_GT/BBOX", "ctc/02_GT/SEG"):
        os.makedirs(tmp_path / d)
    (src / "test.txt").write_text("".join("01/t%03d.tif\n" % k for k in range(70)) + "".join("02/t%03d.tif\n" % k for k in range(3)))
    dets, gtbs = [], []
    for k, (gt, pred, table) in enumerate(imgs):
        rows, lines = [], ["header"]
        for i in np.unique(pred)[1:]:
            z, y, x = np.nonzero(pred == i)
            rows.append([i, x.min(), y.min(), z.min(), x.max(), y.max(), z.max(), table[int(i) - 1, 1]])
        rows = np.array(rows, np.float64)
        for i in np.unique(gt)[1:]:
            z, y, x = np.nonzero(gt == i)
            lines.append("%d %d %d %d %d %d %d %d" % (i, x.min(), y.min(), z.min(), np.ptp(x) + 1, np.ptp(y) + 1, np.ptp(z) + 1, i))
        (src / "02_GT" / "BBOX" / ("bbox_%03d.txt" % k)).write_text("\n".join(lines) + "\n")
        write_tiff_stack(str(src / "02_GT" / "SEG" / ("man_seg%03d.tif" % k)), gt)
        save_detections(str(tmp_path / "dets" / ("02_t%03d.pkl" % k)), [[], rows[:, 1:].astype(np.float32)])
        save_segmentation(str(tmp_path / "seg"), "02_t%03d" % k, pred, rows)
        dets.append(rows)
        gtbs.append(E.load_gt_bbox(str(src / "02_GT" / "BBOX" / ("bbox_%03d.txt" % k)))[0])
    det = E.nuclei_detection_f1(str(tmp_path / "dets"), str(src), str(src / "test.txt"))
    want = E.detection_f1([d[:, 1:].astype(np.float32) for d in dets], gtbs)
    assert det["f1"] == want["f1"] and np.array_equal(det["tp"], want["tp"])
    seg = E.nuclei_segmentation_f1(str(tmp_path / "seg"), str(src), str(src / "test.txt"))
    want_s = E.segmentation_f1([p for _, p, _ in imgs], [g for g, _, _ in imgs], [d[:, 1:7].astype(float) for d in dets], gtbs)
    assert seg["f1"] == want_s["f1"] and seg["tp_pixel"] == want_s["tp_pixel"]
    tool = os.path.join(ROOT, "tools", "evaluate.py")
    run = lambda *a: subprocess.run([sys.executable, tool, *a], capture_output=True, text=True, timeout=300, check=True).stdout
    out = run("soma", str(tmp_path / "pred"), str(tmp_path / "gt"), "--iou-thresh", "0.5")
    assert out.strip().splitlines()[-1] == "ap: {}".format(res["ap"])
    out = run("nuclei-det", str(tmp_path / "dets"), str(src), str(src / "test.txt"))
    assert out.strip() == "done, detection f1 score is {}, precision is {}, recall is {}".format(det["f1"], det["precision"], det["recall"])
    out = run("nuclei-seg", str(tmp_path / "seg"), str(src), str(src / "test.txt"))
    assert out.strip() == "done, instance segmentation f1 score is {:.5f}, precision is {:.5f}, recall is {:.5f}".format(
        seg["f1"], seg["precision"], seg["recall"])
