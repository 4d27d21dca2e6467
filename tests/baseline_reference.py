"""NumPy / SciPy restatement of the reference's tools/evaluation/eval_instance_segmentation_soma_ngps.py, independent of
m3d.evaluate_baselines and of the device: whole-volume labelling with skimage.measure.label's default semantics (on
scipy.ndimage.label), the sphere painting of the NGPS flag, the size filter with its skip-after-remove quirk, and precision / recall /
AP without scores.  The IoU comes from eval_reference's contingency table, so this also runs at full size."""
import numpy as np
from scipy import ndimage

import eval_reference as R

RANK = {6: 1, 18: 2, 26: 3}


def label(x, connectivity=26):
    """(labels int32, K): components of equal non-zero value, numbered by the raster index of their first voxel - scipy.ndimage.label
    once per distinct value, then renumbered (for a binary mask SciPy's own numbering already is that order)."""
    x = np.asarray(x)
    st = ndimage.generate_binary_structure(3, RANK[connectivity])
    vals = np.unique(x)
    vals = vals[vals != 0]
    if len(vals) == 0:
        return np.zeros(x.shape, np.int32), 0
    if len(vals) == 1:
        lab, n = ndimage.label(x == vals[0], structure=st)
        return lab.astype(np.int32), int(n)
    first_all, lab_all, base = [], np.zeros(x.shape, np.int64), 0
    for v in vals:
        lab, n = ndimage.label(x == v, structure=st)
        ids, first = np.unique(lab.ravel(), return_index=True)
        first_all.append(first[ids != 0])
        lab_all += np.where(lab > 0, lab + base, 0)
        base += n
    first_all = np.concatenate(first_all)                  # first_all[j]: first raster index of provisional id j + 1
    new = np.zeros(base + 1, np.int64)
    new[1 + np.argsort(first_all, kind="stable")] = np.arange(1, base + 1)
    return new[lab_all].astype(np.int32), int(base)


def paint_spheres(spheres, shape):
    """:160-183 vectorised per sphere: id i + 1, lower clamp 1, r >= 6, later spheres overwrite."""
    S, H, W = shape
    vol = np.zeros(shape, np.uint16)
    for i, (x, y, z, r) in enumerate(np.asarray(spheres, dtype=np.int64).reshape(-1, 4)):
        x, y, z, r = int(x), int(y), int(z), int(r)
        if r < 6:
            continue
        xs, ys, zs = range(max(1, x - r), min(W, x + r + 1)), range(max(1, y - r), min(H, y + r + 1)), range(max(1, z - r), min(S, z + r + 1))
        if not (len(xs) and len(ys) and len(zs)):
            continue
        zz, yy, xx = np.ogrid[zs[0]:zs[-1] + 1, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        m = (xx - x) ** 2 + (yy - y) ** 2 + (zz - z) ** 2 <= r ** 2
        sub = vol[zs[0]:zs[-1] + 1, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        sub[m] = (i + 1) & 0xFFFF
    return vol


def read_swc(text):
    rows = []
    for line in text.rstrip().split("\n"):
        p = line.rstrip().split(" ")
        rows.append([int(float(p[k])) for k in (2, 3, 4, 5)])
    return np.array(rows, np.int64).reshape(-1, 4)


def select_ids(pred, min_voxels=300):
    """The script's own loop on a Python list (:189-193): removing while iterating skips the element after every removal."""
    ids = np.unique(pred).tolist()
    cnt = np.bincount(np.asarray(pred).ravel().astype(np.int64))
    for m_id in ids:
        if cnt[m_id] < min_voxels:
            ids.remove(m_id)
    ids.remove(0)
    return ids


def prec_rec(preds, gts, iou_thresh, min_voxels=300):
    """-> (prec, rec, ap, per_image_ap, ids): instance-label predictions against GT volumes; no scores, rows in ascending id order."""
    n_pos, match, per, kept = 0, [], [], []
    for pred, gt in zip(preds, gts):
        ids = select_ids(pred, min_voxels)
        kept.append(ids)
        gt_ids = np.unique(gt)
        gt_ids = gt_ids[gt_ids != 0]
        n_pos += len(gt_ids)
        if len(ids) == 0 or len(gt_ids) == 0:
            match.extend([0] * (len(ids) if len(gt_ids) == 0 else 0))
            per.append(np.nan)
            continue
        iou = R.iou_matrix(pred, gt, np.array(ids, np.int64), gt_ids)
        gt_index = iou.argmax(axis=1)
        gt_index[iou.max(axis=1) < iou_thresh] = -1
        selec = np.zeros(len(gt_ids), bool)
        single = []
        for g in gt_index:
            if g >= 0:
                hit = 0 if selec[g] else 1
                match.append(hit)
                single.append(hit)
                selec[g] = True
            else:
                match.append(0)
        ms = np.array(single, np.int8)
        tps, fps = np.cumsum(ms == 1), np.cumsum(ms == 0)
        per.append(R.voc_ap(tps / len(gt_ids), tps / (fps + tps)))
    m = np.array(match, np.int8)
    tp, fp = np.cumsum(m == 1), np.cumsum(m == 0)
    prec, rec = tp / (fp + tp), tp / n_pos
    return prec, rec, R.voc_ap(rec, prec), per, kept
