"""Scoring of instance-label volumes: the figures of the reference's tools/evaluation/ scripts.

  eval_instance_segmentation_soma.py   soma mask AP            -> eval_instance_segmentation_soma / soma_prec_rec
  evaluation_nuclei_f1score.py         nuclei detection F1     -> nuclei_detection_f1 / detection_f1
  evaluation_nuclei_f1score_seg.py     nuclei segmentation F1  -> nuclei_segmentation_f1 / segmentation_f1

The voxel passes run on the device (ops.label_overlap, ops.label_iou_best, ops.box_union_overlap_counts: csrc/eval3d.hip); the
reference builds one full-volume bool mask per instance and loops over P x G x V voxels instead.  The small sequential parts stay
here in NumPy - score sorts, greedy assignment, cumulative sums, voc_ap, the fp64 box IoU - with the reference's operations on
arrays of the same dtypes, so their results carry the reference's bits.  Every score sort is argsort(kind="stable")[::-1]: ties go to
the descending index (SURVEY 8c caveat i; the reference's unstable sort agrees whenever scores are distinct).

Deviations, where the reference fails: an image with predictions but no GT ids (its argmax over an empty axis raises,
eval_instance_segmentation_soma.py:200) counts every row of its score table as a false positive and has a NaN per-image AP; no GT in
any image (NameError, :256) raises ValueError; use_07_metric=True (NameError, :30) raises NotImplementedError; a score-table id 0
(compared against the background, :188) raises ValueError.
"""
import os
import pickle

import numpy as np

from . import ops
from .io import read_tiff_stack

__all__ = ["voc_ap", "calc_instance_segmentation_voc_prec_rec", "eval_instance_segmentation_soma", "load_gt_bbox", "label_iou",
           "nuclei_detection_f1", "nuclei_segmentation_f1", "soma_prec_rec", "detection_f1", "segmentation_f1", "assign_matches",
           "pool_prec_rec", "box_slices", "score_order"]


def score_order(scores):
    """Descending score order; equal scores in descending index order (m3d/binarize.py uses the same rule)."""
    return np.asarray(scores).argsort(kind="stable")[::-1]


# ------------------------------------------------------------------ soma mask AP
def voc_ap(rec, prec, use_07_metric=False):
    """eval_instance_segmentation_soma.py:18-50, all-points form: (mrec, mpre, ap)."""
    if use_07_metric:
        raise NotImplementedError("use_07_metric: the reference's 11-point branch reads mpre before assigning it "
                                  "(eval_instance_segmentation_soma.py:30)")
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]       # the backward running maximum of :39-40 (max is exact: same values)
    i = np.where(mrec[1:] != mrec[:-1])[0]
    ap = np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])
    return mrec, mpre, ap


def _table(table):
    """A soma score table [[mask_id, score], ...] in score order and its integer ids; id 0 or a non-integral id raises ValueError."""
    t = np.asarray(table)
    if t.size == 0:
        t = t.reshape(0, 2)
    if t.ndim != 2 or t.shape[1] < 2:
        raise ValueError("a soma score table has rows [mask_id, score]")
    t = t[score_order(t[:, 1]), :]                                 # :170-171
    ids = t[:, 0]
    if ids.size and (np.any(ids != np.floor(ids)) or ids.min() < 1):
        raise ValueError("score-table ids must be positive integers (id 0 would be compared against the background)")
    return t, ids.astype(np.int64)


def assign_matches(max_iou, argmax, iou_thresh, num_gt):
    """:200-217 on the row maxima: gt_index = argmax, -1 where max < iou_thresh (fp32 against a Python float: NEP 50 compares in
    fp32); then rows in score order claim their GT index, the first claim is a TP (1), later claims and -1 rows are FPs (0).
    A row whose best GT is taken does not fall back to its second best."""
    gt_index = np.asarray(argmax).astype(np.intp)
    gt_index[np.asarray(max_iou) < iou_thresh] = -1
    selec = np.zeros(num_gt, dtype=bool)
    match = []
    for g in gt_index:
        if g >= 0:
            match.append(0 if selec[g] else 1)
            selec[g] = True
        else:
            match.append(0)
    return match


def _prec_rec(scores, match, n_pos):
    match = np.array(match, dtype=np.int8)[score_order(scores)]
    tp = np.cumsum(match == 1)
    fp = np.cumsum(match == 0)
    return tp / (fp + tp), tp / n_pos


def pool_prec_rec(scores, matches, n_pos):
    """:242-258: all images pooled and sorted by score.  n_pos = 0 raises ValueError (the reference: NameError)."""
    if n_pos <= 0:
        raise ValueError("no GT instance in any image: recall is undefined")
    return _prec_rec(np.array(scores), matches, n_pos)


def soma_prec_rec(pred_labels, gt_labels, score_tables, iou_thresh):
    """In-memory core of calc_instance_segmentation_voc_prec_rec: per image a pred label volume, a GT label volume (NumPy or CUDA,
    uint16 / int32) and its score table [[mask_id, score], ...].  Returns (prec, rec, per_image_ap)."""
    tables = [_table(t) for t in score_tables]
    n_pos, scores, matches, per_image = 0, [], [], []
    for pred, gt, (table, ids) in zip(pred_labels, gt_labels, tables):
        scores.extend(table[:, 1])
        ov = ops.label_overlap(pred, gt)
        gt_ids = np.nonzero(ov.count_b[1:].cpu().numpy() > 0)[0] + 1       # :181-182, np.unique minus 0
        n_pos += len(gt_ids)
        if len(table) == 0:                                                  # :189-190
            per_image.append(np.nan)
            continue
        if len(gt_ids) == 0:                                                 # deviation: every row is a FP
            matches.extend([0] * len(table))
            per_image.append(np.nan)
            continue
        best = ops.label_iou_best(ov, ids, gt_ids=gt_ids)
        m = assign_matches(best.max_iou.cpu().numpy(), best.argmax.cpu().numpy(), iou_thresh, len(gt_ids))
        matches.extend(m)
        prec_s, rec_s = _prec_rec(np.array(table[:, 1]), m, len(gt_ids))    # :219-234
        per_image.append(voc_ap(rec_s, prec_s)[2])
    prec, rec = pool_prec_rec(scores, matches, n_pos)
    return prec, rec, per_image


def _read_soma(pred_mask_path, gt_mask_path, img_names):
    preds, gts, tables = [], [], []
    for name in img_names:                                                   # :164-168
        preds.append(read_tiff_stack(os.path.join(pred_mask_path, name + ".tif")))
        gts.append(read_tiff_stack(os.path.join(gt_mask_path, name, name + ".tif")))
        tables.append(np.load(os.path.join(pred_mask_path, name + ".npy")))
    return preds, gts, tables


def calc_instance_segmentation_voc_prec_rec(pred_mask_path, gt_mask_path, img_names, iou_thresh):
    """eval_instance_segmentation_soma.py:107-258: pred/{name}.tif + pred/{name}.npy against gt/{name}/{name}.tif -> (prec, rec)."""
    prec, rec, _ = soma_prec_rec(*_read_soma(pred_mask_path, gt_mask_path, img_names), iou_thresh)
    return prec, rec


def eval_instance_segmentation_soma(pred_mask_path, gt_mask_path, img_names, iou_thresh, use_07_metric=False):
    """eval_instance_segmentation_soma.py:53-104 -> {'ap', 'map', 'per_image_ap'}."""
    if use_07_metric:
        voc_ap(None, None, use_07_metric=True)
    prec, rec, per_image = soma_prec_rec(*_read_soma(pred_mask_path, gt_mask_path, img_names), iou_thresh)
    _, _, ap = voc_ap(rec, prec)
    return {"ap": ap, "map": np.nanmean(ap), "per_image_ap": per_image}


def label_iou(pred_labels, gt_labels, pred_ids=None, gt_ids=None):
    """The dense [P, G] fp32 IoU matrix of `pred_labels == id` against `gt_labels == id` stacks, bit-equal to mask_iou_fast
    (mask_iou.py:50-68).  Default ids: the non-zero labels present, ascending."""
    ov = ops.label_overlap(pred_labels, gt_labels)
    if pred_ids is None:
        pred_ids = np.nonzero(ov.count_a[1:].cpu().numpy() > 0)[0] + 1
    return ops.label_iou_best(ov, np.asarray(pred_ids, dtype=np.int64), gt_ids=gt_ids, dense=True).iou.cpu().numpy()


# ------------------------------------------------------------------ nuclei detection / segmentation F1
def load_gt_bbox(label_file):
    """evaluation_nuclei_f1score.py:18-36: the first line is skipped; rows `i x1 y1 z1 w h s marker` -> boxes float32 [N, 6]
    (x1, y1, z1, x1 + w - 1, ...) and the markers (int64; uint16 when there is no row, as np.append leaves them)."""
    with open(label_file, "r") as f:
        lines = f.readlines()
    boxes, markers = [], []
    for line in lines[1:]:
        p = line.rstrip().split(" ")
        x1, y1, z1 = int(p[1]), int(p[2]), int(p[3])
        boxes.append((x1, y1, z1, x1 + int(p[4]) - 1, y1 + int(p[5]) - 1, z1 + int(p[6]) - 1))
        markers.append(int(p[7]))
    gt = np.array(boxes, dtype=np.float32).reshape(-1, 6)
    return gt, (np.array(markers, dtype=np.int64) if markers else np.empty(0, dtype=np.uint16))


def _box_overlaps(bb, gt):
    """evaluation_nuclei_f1score.py:136-153 in its operation order (bb: one box, gt: [G, 6]; fp64 when both are)."""
    ixmin = np.maximum(gt[:, 0], bb[0])
    iymin = np.maximum(gt[:, 1], bb[1])
    izmin = np.maximum(gt[:, 2], bb[2])
    ixmax = np.minimum(gt[:, 3], bb[3])
    iymax = np.minimum(gt[:, 4], bb[4])
    izmax = np.minimum(gt[:, 5], bb[5])
    iw = np.maximum(ixmax - ixmin + 1., 0.)
    ih = np.maximum(iymax - iymin + 1., 0.)
    iss = np.maximum(izmax - izmin + 1., 0.)
    inters = iw * ih * iss
    uni = ((bb[3] - bb[0] + 1.) * (bb[4] - bb[1] + 1.) * (bb[5] - bb[2] + 1.) +
           (gt[:, 3] - gt[:, 0] + 1.) * (gt[:, 4] - gt[:, 1] + 1.) * (gt[:, 5] - gt[:, 2] + 1.) - inters)
    return inters / uni


def _f1(tp_sum, npos, nd):
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = tp_sum / npos
        precision = tp_sum / nd
        f1 = 2 * (recall * precision) / (recall + precision)
    return f1, precision, recall


def detection_f1(dets, gt_boxes, ovthresh=0.4, score_thresh=0.4):
    """In-memory core of evaluation_nuclei_f1score.py:95-169.  dets: per image the detection rows (7 columns: box + score, or 8:
    id + box + score); gt_boxes: per image float32 [G, 6].  Rows with score > score_thresh are kept (:110; fp32 scores compare in
    fp32) and processed in file order, not by confidence; a row is a TP when its best IoU over ALL GT boxes of its image is
    > ovthresh and that box is not yet detected.  Returns dict(f1, precision, recall, tp, fp); nd = 0 gives NaN."""
    npos = sum(int(np.asarray(g).shape[0]) for g in gt_boxes)
    tp, fp = [], []
    for res, gt in zip(dets, gt_boxes):
        res = np.asarray(res)
        res = res[res[:, -1] > score_thresh, :]
        if res.shape[1] == 7:
            bbs = res[:, :6]
        elif res.shape[1] == 8:
            bbs = res[:, 1:7]
        else:
            raise ValueError("detection rows have 7 or 8 columns, got %d" % res.shape[1])
        gtf = np.asarray(gt).astype(float)
        det = np.zeros(gtf.shape[0], dtype=bool)
        for d in range(bbs.shape[0]):
            bb = bbs[d, :].astype(float)
            ovmax, jmax = -np.inf, 0
            if gtf.size > 0:
                ov = _box_overlaps(bb, gtf)
                ovmax, jmax = np.max(ov), np.argmax(ov)
            if ovmax > ovthresh and not det[jmax]:
                tp.append(1.), fp.append(0.)
                det[jmax] = 1
            else:
                tp.append(0.), fp.append(1.)
    tp, fp = np.array(tp, dtype=np.float64), np.array(fp, dtype=np.float64)
    f1, precision, recall = _f1(np.sum(tp), npos, len(tp))
    return dict(f1=f1, precision=precision, recall=recall, tp=tp, fp=fp)


def box_slices(bbox, shape):
    """The voxels `keep[z1:z2+1, y1:y2+1, x1:x2+1]` addresses (evaluation_nuclei_f1score_seg.py:126-127, bbox.astype(int)
    truncates) under NumPy slice semantics - ends clipped, negative starts wrap - as half-open (z0, z1, y0, y1, x0, x1)."""
    x1, y1, z1, x2, y2, z2 = np.asarray(bbox)[:6].astype(int)
    out = []
    for lo, hi, n in ((z1, z2, shape[0]), (y1, y2, shape[1]), (x1, x2, shape[2])):
        s, e, _ = slice(int(lo), int(hi) + 1).indices(int(n))
        out += [s, max(s, e)]
    return tuple(out)


def segmentation_f1(pred_labels, gt_labels, det_boxes, gt_boxes, ovthresh=0.4):
    """In-memory core of evaluation_nuclei_f1score_seg.py:65-141.  det_boxes: per image [N, >= 6] boxes (x1, y1, z1, x2, y2, z2 first,
    used in their own dtype as the script does), no score filter; the TP boxes' union picks the predicted voxels that count.
    Returns dict(f1, precision, recall, tp_pixel, gt_pixel, pre_pixel)."""
    tp_pixel, gt_pixel, pre_pixel = np.int64(0), np.int64(0), np.int64(0)
    for pred, gt, dets, gtb in zip(pred_labels, gt_labels, det_boxes, gt_boxes):
        gtf = np.asarray(gtb).astype(float)
        ranges = []
        if gtf.shape[0] > 0:
            detected = np.zeros(gtf.shape[0], dtype=bool)
            for bbox in np.asarray(dets):
                ov = _box_overlaps(bbox, gtf)
                ovmax, jmax = np.max(ov), np.argmax(ov)
                if ovmax > ovthresh and not detected[jmax]:
                    detected[jmax] = 1
                    ranges.append(box_slices(bbox, tuple(pred.shape)))
        pre, gtp, tpp = ops.box_union_overlap_counts(pred, gt, np.array(ranges, dtype=np.int64).reshape(-1, 6))
        gt_pixel += gtp
        pre_pixel += pre
        if gtf.shape[0] > 0:
            tp_pixel += tpp
    with np.errstate(divide="ignore", invalid="ignore"):
        recall = tp_pixel / gt_pixel
        precision = tp_pixel / pre_pixel
        f1 = 2 * (recall * precision) / (recall + precision)
    return dict(f1=f1, precision=precision, recall=recall, tp_pixel=tp_pixel, gt_pixel=gt_pixel, pre_pixel=pre_pixel)


def _test_images(test_txt, track):
    with open(test_txt, "r") as f:
        paths = [x.rstrip() for x in f.readlines()]
    if track == "01":
        paths = paths[:70]
    elif track == "02":
        paths = paths[70:]
    return [(p.split("/")[-2], p.split("/")[-2] + "_" + p.split("/")[-1][:-4]) for p in paths]


def nuclei_detection_f1(res_path, src_path, test_txt, track="02", ovthresh=0.4, score_thresh=0.4, save_as_pkl=True):
    """evaluation_nuclei_f1score.py as a function (its module constants are the parameters): {res_path}/{name}.pkl (or .npy) against
    {src_path}/{track}_GT/BBOX/bbox_NNN.txt for the images of test_txt (track '02': entries 70 on)."""
    dets, gts = [], []
    for trk, name in _test_images(test_txt, track):
        gts.append(load_gt_bbox(os.path.join(src_path, trk + "_GT", "BBOX", "bbox_" + name[-3:] + ".txt"))[0])
        if save_as_pkl:
            with open(os.path.join(res_path, name + ".pkl"), "rb") as f:
                dets.append(pickle.load(f)["all_boxes"][1])
        else:
            dets.append(np.load(os.path.join(res_path, name + ".npy")))
    return detection_f1(dets, gts, ovthresh, score_thresh)


def nuclei_segmentation_f1(res_path, src_path, test_txt, track="02", ovthresh=0.4, save_as_pkl=False):
    """evaluation_nuclei_f1score_seg.py as a function: {res_path}/{name}.tif + {name}.npy (rows [id, x1, y1, z1, x2, y2, z2, score])
    against {src_path}/{track}_GT/SEG/man_segNNN.tif and the BBOX files."""
    preds, gts, dets, gtbs = [], [], [], []
    for trk, name in _test_images(test_txt, track):
        gtbs.append(load_gt_bbox(os.path.join(src_path, trk + "_GT", "BBOX", "bbox_" + name[-3:] + ".txt"))[0])
        if save_as_pkl:
            with open(os.path.join(res_path, name + ".pkl"), "rb") as f:
                dets.append(pickle.load(f)["all_boxes"][1])
        else:
            dets.append(np.load(os.path.join(res_path, name + ".npy"))[:, 1:7].astype(float))
        gts.append(read_tiff_stack(os.path.join(src_path, trk + "_GT", "SEG", "man_seg" + name[-3:] + ".tif")))
        preds.append(read_tiff_stack(os.path.join(res_path, name + ".tif")))
    return segmentation_f1(preds, gts, dets, gtbs, ovthresh)
