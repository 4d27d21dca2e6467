"""NumPy restatement of the four computations of the reference's tools/evaluation/ scripts, independent of m3d.evaluate and of the
device: mask_iou_fast (mask_iou.py:50-68), the soma AP (eval_instance_segmentation_soma.py:18-258), the nuclei detection F1
(evaluation_nuclei_f1score.py:95-169) and the nuclei segmentation F1 (evaluation_nuclei_f1score_seg.py:65-141).  The IoU comes from a
contingency table of (pred id, GT id) voxel counts (np.unique on combined keys) instead of one bool mask per instance, so this also
runs at full size.  Score sorts use argsort(kind="stable")[::-1]."""
import numpy as np


def contingency(a, b):
    """(count_a, count_b, pairs int64 [P, 2] sorted by (a, b) with a > 0 and b > 0, counts int64 [P])"""
    a = np.asarray(a).astype(np.int64).ravel()
    b = np.asarray(b).astype(np.int64).ravel()
    key, cnt = np.unique(a * (1 << 24) + b, return_counts=True)
    pa, pb = key >> 24, key & ((1 << 24) - 1)
    keep = (pa > 0) & (pb > 0)
    return np.bincount(a), np.bincount(b), np.stack([pa[keep], pb[keep]], 1), cnt[keep].astype(np.int64)


def iou_matrix(pred, gt, pred_ids, gt_ids):
    """mask_iou_fast(pred == id stack, gt == id stack): float32(double(inter) / double(|a| + |b| - inter))."""
    ca, cb, pairs, cnt = contingency(pred, gt)
    na = np.array([ca[i] if i < len(ca) else 0 for i in pred_ids], np.float64)
    nb = np.array([cb[i] if i < len(cb) else 0 for i in gt_ids], np.float64)
    inter = np.zeros((len(pred_ids), len(gt_ids)), np.float64)
    row = {int(v): k for k, v in enumerate(pred_ids)}
    col = {int(v): k for k, v in enumerate(gt_ids)}
    for (x, y), c in zip(pairs, cnt):
        if int(x) in row and int(y) in col:
            inter[row[int(x)], col[int(y)]] = c
    return (inter / (na[:, None] + nb[None, :] - inter)).astype(np.float32)


def voc_ap(rec, prec):
    mrec = np.concatenate(([0.], rec, [1.]))
    mpre = np.concatenate(([0.], prec, [0.]))
    for i in range(mpre.size - 1, 0, -1):
        mpre[i - 1] = np.maximum(mpre[i - 1], mpre[i])
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])


def soma(preds, gts, tables, iou_thresh):
    """-> (prec, rec, ap, per_image_ap); images without predictions get a NaN per-image AP."""
    n_pos, score, match, per = 0, [], [], []
    for pred, gt, t in zip(preds, gts, tables):
        t = np.asarray(t).reshape(-1, 2)
        t = t[t[:, 1].argsort(kind="stable")[::-1], :]
        score.extend(t[:, 1])
        gt_ids = np.unique(gt)
        gt_ids = gt_ids[gt_ids != 0]
        n_pos += len(gt_ids)
        if len(t) == 0:
            per.append(np.nan)
            continue
        if len(gt_ids) == 0:
            match.extend([0] * len(t))
            per.append(np.nan)
            continue
        iou = iou_matrix(pred, gt, t[:, 0].astype(np.int64), gt_ids)
        gt_index = iou.argmax(axis=1)
        gt_index[iou.max(axis=1) < iou_thresh] = -1
        selec = np.zeros(len(gt_ids), bool)
        m = []
        for g in gt_index:
            m.append(int(g >= 0 and not selec[g]))
            if g >= 0:
                selec[g] = True
        match.extend(m)
        ms = np.array(m, np.int8)[np.array(t[:, 1]).argsort(kind="stable")[::-1]]
        tps, fps = np.cumsum(ms == 1), np.cumsum(ms == 0)
        per.append(voc_ap(tps / len(gt_ids), tps / (fps + tps)))
    match = np.array(match, np.int8)[np.array(score).argsort(kind="stable")[::-1]]
    tp, fp = np.cumsum(match == 1), np.cumsum(match == 0)
    prec, rec = tp / (fp + tp), tp / n_pos
    return prec, rec, voc_ap(rec, prec), per


def _overlaps(bb, g):
    iw = np.maximum(np.minimum(g[:, 3], bb[3]) - np.maximum(g[:, 0], bb[0]) + 1., 0.)
    ih = np.maximum(np.minimum(g[:, 4], bb[4]) - np.maximum(g[:, 1], bb[1]) + 1., 0.)
    iz = np.maximum(np.minimum(g[:, 5], bb[5]) - np.maximum(g[:, 2], bb[2]) + 1., 0.)
    inters = iw * ih * iz
    uni = ((bb[3] - bb[0] + 1.) * (bb[4] - bb[1] + 1.) * (bb[5] - bb[2] + 1.) +
           (g[:, 3] - g[:, 0] + 1.) * (g[:, 4] - g[:, 1] + 1.) * (g[:, 5] - g[:, 2] + 1.) - inters)
    return inters / uni


def detection(dets, gt_boxes, ovthresh=0.4, score_thresh=0.4):
    """-> (f1, precision, recall, tp, fp)"""
    npos = sum(len(g) for g in gt_boxes)
    tp, fp = [], []
    for res, g in zip(dets, gt_boxes):
        res = np.asarray(res)
        res = res[res[:, -1] > score_thresh]
        bbs = res[:, :6] if res.shape[1] == 7 else res[:, 1:7]
        g = np.asarray(g).astype(float)
        seen = np.zeros(len(g), bool)
        for bb in bbs.astype(float):
            ov = _overlaps(bb, g) if len(g) else np.array([-np.inf])
            j = int(np.argmax(ov))
            hit = ov[j] > ovthresh and not seen[j]
            tp.append(float(hit))
            fp.append(float(not hit))
            if hit:
                seen[j] = True
    tp, fp = np.array(tp), np.array(fp)
    with np.errstate(divide="ignore", invalid="ignore"):
        r, p = np.sum(tp) / npos, np.sum(tp) / len(tp)
        return 2 * (r * p) / (r + p), p, r, tp, fp


def segmentation(preds, gts, det_boxes, gt_boxes, ovthresh=0.4):
    """-> (f1, precision, recall, tp_pixel, gt_pixel, pre_pixel), the TP boxes painted with NumPy slicing as the script does"""
    tpp = gtp = prp = np.int64(0)
    for pred, gt, dets, g in zip(preds, gts, det_boxes, gt_boxes):
        g = np.asarray(g).astype(float)
        pb, gb = pred > 0, gt > 0
        gtp += np.sum(gb)
        prp += np.sum(pb)
        if len(g) == 0:
            continue
        keep = np.zeros(pred.shape, bool)
        seen = np.zeros(len(g), bool)
        for bb in np.asarray(dets):
            ov = _overlaps(bb, g)
            j = int(np.argmax(ov))
            if ov[j] > ovthresh and not seen[j]:
                seen[j] = True
                x1, y1, z1, x2, y2, z2 = bb[:6].astype(int)
                keep[z1:z2 + 1, y1:y2 + 1, x1:x2 + 1] = pb[z1:z2 + 1, y1:y2 + 1, x1:x2 + 1]
        tpp += np.sum(keep & gb)
    with np.errstate(divide="ignore", invalid="ignore"):
        r, p = tpp / gtp, tpp / prp
        return 2 * (r * p) / (r + p), p, r, tpp, gtp, prp
