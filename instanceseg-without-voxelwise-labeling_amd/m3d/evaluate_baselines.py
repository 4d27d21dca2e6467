"""Scoring of the two baselines the soma results are compared with: the reference's tools/evaluation/
eval_instance_segmentation_soma_ngps.py, whose function names and flag-first signatures are kept.

  flag 'DSN'   pred/{name}.tif is a voxelwise segmentation; its connected components (skimage.measure.label, full connectivity)
               are the instances                                        -> ops.label_components (csrc/label3d.hip)
  flag 'NGPS'  pred/{name}.swc is a NeuroGPS soma list; every line is painted as a sphere into a uint16 volume
                                                                        -> read_swc_spheres, ops.paint_spheres

The voxel work runs on the device: labelling or painting, then the contingency table and the IoU maxima of m3d.evaluate's path
(ops.label_overlap, ops.label_iou_best).  The per-label voxel counts of the size filter are Overlap.count_a.  The sequential parts
are the NumPy steps of m3d.evaluate (voc_ap, assign_matches, the cumulative precision / recall), imported, not copied.

Behaviour of the script that is reproduced on purpose:
  * the size filter (:189-193) removes from the list it iterates over, so the element after every removed id is never tested and
    survives whatever its size: select_pred_ids.  Then `ids.remove(0)`: a prediction without background voxels, or with fewer than
    min_voxels of them, raises ValueError there, and so does this module (and a GT volume without background, :195);
  * there are no scores: rows are the surviving ids in ascending order, precision and recall are cumulative over that order, the
    images concatenated;
  * the pooled `match` and the per-image `match_single` differ (:219-229): a row without a GT above the threshold appends 0 to
    `match` only, a row whose GT is already taken appends 0 to both;
  * SWC fields are `line.rstrip().split(' ')[2:6]`, each int(float(.)) - truncation toward zero; the id counter advances for every
    line, those with r < 6 included, which paint nothing.

Deviations, where the script fails: an image with predictions but no GT ids (argmax over an empty axis, :213) counts its rows as false
positives and has a NaN per-image AP; no GT in any image (NameError, :258) raises ValueError; use_07_metric=True (NameError, :27)
raises NotImplementedError through m3d.evaluate.voc_ap; an empty SWC file, or a line with fewer than six fields (IndexError, :169-172),
raises ValueError.  An image without surviving predictions has a NaN per-image AP (the script computes none, :202-203).
"""
import os

import numpy as np

from . import ops
from .evaluate import voc_ap, assign_matches, pool_prec_rec, _prec_rec
from .io import read_tiff_stack

__all__ = ["calc_instance_segmentation_voc_prec_rec", "eval_instance_segmentation_soma", "baseline_prec_rec", "read_swc_spheres",
           "select_pred_ids", "FLAGS"]

FLAGS = ("DSN", "NGPS")


def select_pred_ids(ids, counts, min_voxels=300):
    """:189-193 exactly.  ids: the ascending values present in the prediction (np.unique, 0 included when there is background);
    counts[id]: its voxels.  `for m_id in ids: if count < min_voxels: ids.remove(m_id)` skips the element after every removal; then
    ids.remove(0) raises ValueError when 0 is absent or was removed.  Returns the surviving ids as a list of int."""
    ids = [int(i) for i in ids]
    i = 0
    while i < len(ids):                    # a list iterator: the index advances by one whether or not the list shrank
        if counts[ids[i]] < min_voxels:
            del ids[i]                     # ids are distinct: remove(m_id) deletes position i
        i += 1
    if 0 not in ids:
        raise ValueError("the prediction has no background id 0 with at least %d voxels (list.remove(0) fails in the reference)"
                         % min_voxels)
    ids.remove(0)
    return ids


def read_swc_spheres(path):
    """:162-172: one sphere per line, (x, y, z, r) = fields 2..5 of `line.rstrip().split(' ')`, each int(float(.)).  int64 [N, 4];
    row i is mask id i + 1.  An empty file or a short line raises ValueError."""
    with open(path, "r") as f:
        lines = f.read().rstrip().split("\n")
    out = []
    for k, line in enumerate(lines):
        p = line.rstrip().split(" ")
        if len(p) < 6:
            raise ValueError("%s line %d: an SWC line has at least six space-separated fields" % (path, k + 1))
        out.append([int(float(p[2])), int(float(p[3])), int(float(p[4])), int(float(p[5]))])
    return np.array(out, dtype=np.int64).reshape(-1, 4)


def baseline_prec_rec(pred_labels, gt_labels, iou_thresh, min_voxels=300):
    """In-memory core of calc_instance_segmentation_voc_prec_rec (:154-258): per image an instance-label volume of the prediction
    (what ops.label_components or ops.paint_spheres return; NumPy or CUDA) and a GT label volume.
    Returns (prec, rec, per_image_ap, pred_ids): pred_ids[k] = the rows of image k, the ids that survive select_pred_ids."""
    n_pos, match, per_image, kept = 0, [], [], []
    for pred, gt in zip(pred_labels, gt_labels):
        ov = ops.label_overlap(pred, gt)
        count_a = ov.count_a.cpu().numpy()
        count_b = ov.count_b.cpu().numpy()
        ids = select_pred_ids(np.nonzero(count_a > 0)[0], count_a, min_voxels)          # np.unique(pred_mask) and :190-193
        if count_b[0] == 0:
            raise ValueError("the GT volume has no background id 0 (list.remove(0) fails in the reference, :195)")
        gt_ids = np.nonzero(count_b[1:] > 0)[0] + 1
        kept.append(np.array(ids, dtype=np.int64))
        n_pos += len(gt_ids)
        if len(ids) == 0:                                                                # :202-203
            per_image.append(np.nan)
            continue
        if len(gt_ids) == 0:                                                             # deviation: every row is a FP
            match.extend([0] * len(ids))
            per_image.append(np.nan)
            continue
        best = ops.label_iou_best(ov, np.array(ids, dtype=np.int64), gt_ids=gt_ids)
        max_iou = best.max_iou.cpu().numpy()
        m = assign_matches(max_iou, best.argmax.cpu().numpy(), iou_thresh, len(gt_ids))
        match.extend(m)
        # match_single leaves out the rows without a GT above the threshold (:228-229 appends to `match` only)
        single = [v for v, none in zip(m, max_iou < iou_thresh) if not none]
        prec_s, rec_s = _prec_rec(-np.arange(len(single), dtype=np.float64), single, len(gt_ids))    # row order kept
        per_image.append(voc_ap(rec_s, prec_s)[2])
    prec, rec = pool_prec_rec(-np.arange(len(match), dtype=np.float64), match, n_pos)
    return prec, rec, per_image, kept


def _read(flag, pred_mask_path, gt_mask_path, img_names):
    if flag not in FLAGS:
        raise ValueError("flag must be 'DSN' or 'NGPS', got %r" % (flag,))
    preds, gts = [], []
    for name in img_names:
        gt = read_tiff_stack(os.path.join(gt_mask_path, name, name + ".tif"))            # :158
        if flag == "NGPS":
            pred = ops.paint_spheres(read_swc_spheres(os.path.join(pred_mask_path, name + ".swc")), gt.shape)
        else:
            pred = ops.label_components(read_tiff_stack(os.path.join(pred_mask_path, name + ".tif")))[0]   # :185-186
        preds.append(pred)
        gts.append(gt)
    return preds, gts


def calc_instance_segmentation_voc_prec_rec(flag, pred_mask_path, gt_mask_path, img_names, iou_thresh):
    """eval_instance_segmentation_soma_ngps.py:102-258: flag 'DSN' pred/{name}.tif, flag 'NGPS' pred/{name}.swc, against
    gt/{name}/{name}.tif -> (prec, rec)."""
    prec, rec, _, _ = baseline_prec_rec(*_read(flag, pred_mask_path, gt_mask_path, img_names), iou_thresh)
    return prec, rec


def eval_instance_segmentation_soma(flag, pred_mask_path, gt_mask_path, img_names, iou_thresh, use_07_metric=False):
    """eval_instance_segmentation_soma_ngps.py:48-99 -> {'ap', 'map', 'per_image_ap'}."""
    if use_07_metric:
        voc_ap(None, None, use_07_metric=True)
    prec, rec, per_image, _ = baseline_prec_rec(*_read(flag, pred_mask_path, gt_mask_path, img_names), iou_thresh)
    _, _, ap = voc_ap(rec, prec)
    return {"ap": ap, "map": np.nanmean(ap), "per_image_ap": per_image}
