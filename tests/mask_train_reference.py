"""NumPy restatement of the mask-branch training step (the checker of tests/test_mask_train_host.py and tests/test_gpu_mask_train.py):
the M^3 targets of lib/roi_data/mask_rcnn.py in two forms, spots_to_boxes, the assignment, the class-specific expansion, and the mask
loss with its gradient.  Written from the description in DESIGN ("Mask-branch training targets"); tests/golden/gen_mask_train.py checks
it against the reference's own add_mask_rcnn_blobs / mask_rcnn_losses.

  direct form   the reference's fill (segms.py:141-146 / :188-189), oracle.skimage_resize_nd, > 0
  closed form   per-axis footprint intervals, the nearest-integer sphere test, the separable interval-"any"; what the kernel computes

The two are not the same function.  The closed form is "resize > 0" with the resize carried out in fp64 (`fp64=True` of the direct
form: resize_nd_fp64): every term is a product of non-negative weights and 0/1 voxels, so the sign is a set predicate.  The reference's
resize writes fp32, and a product below 2^-150 underflows to 0 there.  At M = 14 that happens where the fp64 coordinate of an output
index lands a few 1e-15 beside an integer (tiny_corners: 42 lengths up to 1024, the first 18, 34, 58, 82) - one corner then has a
weight near 2e-15, which counts on its own but not times the Gaussian tails of the other axes (2.3e-11 at n = 18).  There the closed
form sets voxels the reference leaves 0; it never misses one the reference sets (DESIGN, "Mask-branch training targets").

Axes are (z, y, x) = (slices, height, width); boxes are (x1, y1, z1, x2, y2, z2)."""
import math

import numpy as np

from rpn_train_reference import overlaps

f32, f64 = np.float32, np.float64
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
MAX_EXTENT = 1024          # the device clamps RoI extents to [2, 1024]


# ---------------------------------------------------------------- footprints of resize(.) > 0
def mirror(j, n):
    """scipy.ndimage's 'mirror' boundary: reflect about the centres of the edge samples, period 2 (n - 1)"""
    p = 2 * (n - 1)
    j %= p
    return p - j if j > n - 1 else j


def interval_table(n, M):
    """(lo[M], hi[M]): output index i of resize(e, (M,)) > 0 is True exactly for unit impulses e at source indices lo[i] .. hi[i].
    Gaussian of sigma = max(0, (n / M - 1) / 2) with radius int(4 sigma + 0.5) (skipped for sigma <= 1e-15), then the order-1 corners of
    the fp64 coordinate n / M (i + 0.5) - 0.5, the upper corner only with a weight that is not exactly 0; mirror boundary throughout."""
    n, M = int(n), int(M)
    fac = f64(n) / f64(M)
    sigma = max(0.0, (float(fac) - 1.0) / 2.0)
    lw = int(4.0 * sigma + 0.5) if sigma > 1e-15 else 0
    lo, hi = np.zeros(M, np.int32), np.zeros(M, np.int32)
    for i in range(M):
        c = float(fac * (f64(i) + 0.5) - 0.5)
        if c < 0.0:
            c = -c
        if c > n - 1:
            c = (2 * n - 2) - c
        c0 = int(math.floor(c))
        top = c0 + 1 if (c - c0) != 0.0 else c0
        js = [mirror(j, n) for j in range(c0 - lw, top + lw + 1)]
        lo[i], hi[i] = min(js), max(js)
    return lo, hi


def tiny_corners(n, M, below=1e-9):
    """the output indices of an axis one of whose two interpolation corners has a weight in (0, below) - the fp64 coordinate lies a
    few 1e-15 above or below an integer: the lengths where the reference's fp32 resize can underflow"""
    fac = f64(n) / f64(M)
    out = []
    for i in range(int(M)):
        c = float(fac * (f64(i) + 0.5) - 0.5)
        c = -c if c < 0.0 else c
        c = (2 * n - 2) - c if c > n - 1 else c
        t = c - math.floor(c)
        if 0.0 < t < below or 0.0 < 1.0 - t < below:
            out.append(i)
    return out


def resize_nd_fp64(image, output_shape):
    """oracle.skimage_resize_nd's steps on an fp64 image with fp64 results: the same algorithm without the fp32 underflow"""
    from scipy import ndimage as ndi
    image = np.asarray(image, f64)
    output_shape = tuple(int(v) for v in output_shape)
    factors = np.asarray(image.shape, f64) / np.asarray(output_shape, f64)
    image = ndi.gaussian_filter(image, np.maximum(0, (factors - 1) / 2), cval=0, mode="mirror")
    coords = [factors[i] * (np.arange(d) + 0.5) - 0.5 for i, d in enumerate(output_shape)]
    return ndi.map_coordinates(image, np.array(np.meshgrid(*coords, sparse=False, indexing="ij")), order=1, mode="mirror", cval=0)


def resize_positive(v, M, fp64=False):
    if fp64:
        return resize_nd_fp64(v, (M, M, M)) > 0
    from oracle import skimage_resize_nd
    return skimage_resize_nd(np.asarray(v, f32), (M, M, M)) > 0


_tables = {}


def table(n, M):
    if (n, M) not in _tables:
        _tables[(n, M)] = interval_table(n, M)
    return _tables[(n, M)]


def impulse_table(n, M):
    """bool [M, n]: the definition - which unit impulses reach which output of the resize"""
    from oracle import skimage_resize_nd
    F = np.zeros((M, n), bool)
    for j in range(n):
        e = np.zeros((n,), f32)
        e[j] = 1
        F[:, j] = skimage_resize_nd(e, (M,)) > 0
    return F


# ---------------------------------------------------------------- boxes and assignment
def spots_to_boxes(spots, in_size):
    """segms.py:209-225 on fp32 spots (x, y, z, r): c -+ (r - 1), clipped to the tile; Python's max / min keep their first argument
    unless the second is strictly beyond it"""
    sp = np.asarray(spots, f32).reshape(-1, 4)
    S, H, W = [int(v) for v in in_size]
    out = np.zeros((len(sp), 6), f32)
    for i, s in enumerate(sp):
        for a, top in enumerate((W - 1, H - 1, S - 1)):
            lo = (s[a] - s[3]) + f32(1)
            hi = (s[a] + s[3]) - f32(1)
            out[i, a] = lo if lo > 0 else 0
            out[i, 3 + a] = hi if hi < top else top
    return out


def eligible(K, classes=None, crowd=None):
    classes = np.ones(K, np.int32) if classes is None else np.asarray(classes, np.int32).reshape(K)
    crowd = np.zeros(K, bool) if crowd is None else np.asarray(crowd).astype(bool).reshape(K)
    return np.flatnonzero((classes > 0) & ~crowd)


def assign(rois_fg, boxes, classes=None, crowd=None):
    """mask_rcnn.py:41-70: per fg RoI the first arg-max of the IoU over the objects with class > 0 that are not crowd, as an index
    into the image's own object list (all-zero overlaps choose the first such object; none at all: -1)"""
    rois_fg = np.asarray(rois_fg, f32).reshape(-1, 6)
    el = eligible(len(boxes), classes, crowd)
    if not len(el) or not len(rois_fg):
        return np.full(len(rois_fg), -1, np.int32)
    return el[overlaps(rois_fg, np.asarray(boxes, f32).reshape(-1, 6)[el]).argmax(1)].astype(np.int32)


# ---------------------------------------------------------------- spot mode
def spot_geometry(spot, box):
    """extents (S, H, W), centre (z, y, x) and radius of segms.py:126-141, all fp32; extents clamped as the device clamps them"""
    sp, box = np.asarray(spot, f32), np.asarray(box, f32)
    ext = []
    for a in (2, 1, 0):
        e = box[3 + a] - box[a]
        e = e if e >= 2 else f32(2)
        ext.append(int(min(e, f32(MAX_EXTENT))))
    ctr = [sp[2] - box[2], sp[1] - box[1], sp[0] - box[0]]
    return tuple(ext), ctr, sp[3]


def spot_mask_direct(spot, box, M, fp64=False):
    """the fill of segms.py:141-146 in fp32 (differences, squares, a left-to-right sum), the resize (the reference's fp32 one, or with
    fp64 the same steps in fp64), > 0"""
    (S, H, W), (z, y, x), r = spot_geometry(spot, box)
    i = np.arange(S, dtype=f32)[:, None, None]
    j = np.arange(H, dtype=f32)[None, :, None]
    k = np.arange(W, dtype=f32)[None, None, :]
    m = ((((i - z) * (i - z) + (j - y) * (j - y)) + (k - x) * (k - x)) < r * r).astype(f32)
    return resize_positive(m, M, fp64).astype(np.int32)


def axis_min(c, lo, hi):
    """per output index the smallest fp32 (t - c)^2 over the integers t of [lo, hi]: reached at an end or next to c"""
    out = np.empty(len(lo), f32)
    fl = np.floor(c)
    for q in range(len(lo)):
        cands = [f32(lo[q]), f32(hi[q])]
        for t in (fl, fl + f32(1)):
            if t >= f32(lo[q]) and t <= f32(hi[q]):
                cands.append(f32(t))
        d = np.array(cands, f32) - c
        out[q] = (d * d).min()
    return out


def spot_mask_closed(spot, box, M):
    (S, H, W), (z, y, x), r = spot_geometry(spot, box)
    with np.errstate(invalid="ignore", over="ignore"):
        dz, dy, dx = axis_min(z, *table(S, M)), axis_min(y, *table(H, M)), axis_min(x, *table(W, M))
        return (((dz[:, None, None] + dy[None, :, None]) + dx[None, None, :]) < r * r).astype(np.int32)


# ---------------------------------------------------------------- mask mode
def trunc_box(b):
    return np.clip(np.asarray(b, f32), -2.0 ** 29, 2.0 ** 29).astype(np.int64)       # astype(int): towards zero


def label_region(box_gt, box, dims):
    """extents (S, H, W) of the integer RoI, its origin (z, y, x) and the copied region [r1, r2) per axis in tile coordinates
    (segms.py:158-189), cut to the RoI's clamped extent and to the volume; an empty intersection copies nothing"""
    bi, bg = trunc_box(box), trunc_box(box_gt)
    ext, org, reg = [], [], []
    for a, dim in zip((2, 1, 0), dims):
        e = int(min(max(bi[3 + a] - bi[a], 2), MAX_EXTENT))
        r1 = max(bi[a], bg[a], 0)
        r2 = min(bi[3 + a], bg[3 + a], bi[a] + e, int(dim))
        ext.append(e)
        org.append(int(bi[a]))
        reg.append((int(r1), int(max(r2, r1))))
    return tuple(ext), tuple(org), reg


def roi_volume(labels, marker, box_gt, box):
    (S, H, W), (oz, oy, ox), ((z1, z2), (y1, y2), (x1, x2)) = label_region(box_gt, box, labels.shape)
    v = np.zeros((S, H, W), bool)
    v[z1 - oz:z2 - oz, y1 - oy:y2 - oy, x1 - ox:x2 - ox] = labels[z1:z2, y1:y2, x1:x2] == marker
    return v


def label_mask_direct(labels, marker, box_gt, box, M, fp64=False):
    return resize_positive(roi_volume(labels, marker, box_gt, box).astype(f32), M, fp64).astype(np.int32)


def interval_any(v, axis, lo, hi):
    """out[.., i, ..] = any of v over [lo[i], hi[i]] along `axis`, through a prefix count"""
    c = np.cumsum(np.moveaxis(v, axis, 0).astype(np.int64), 0)
    c = np.concatenate([np.zeros((1,) + c.shape[1:], np.int64), c], 0)
    return np.moveaxis((c[np.asarray(hi) + 1] - c[np.asarray(lo)]) > 0, 0, axis)


def label_mask_closed(labels, marker, box_gt, box, M):
    v = roi_volume(labels, marker, box_gt, box)
    for axis in (2, 1, 0):                       # x, then y, then z
        v = interval_any(v, axis, *table(v.shape[axis], M))
    return v.astype(np.int32)


# ---------------------------------------------------------------- the blobs of one image
def expand(masks, classes, num_classes, M):
    """_expand_to_class_specific_mask_targets (mask_rcnn.py:115-135)"""
    out = -np.ones((len(masks), num_classes * M ** 3), np.int32)
    for i, c in enumerate(np.asarray(classes).astype(np.int64)):
        if 0 < c < num_classes:
            out[i, M ** 3 * c:M ** 3 * (c + 1)] = masks[i]
    return out


def mask_targets(labels_int32, rois, M, form="closed", spots=None, in_size=None, gt_boxes=None, markers=None, label_volume=None,
                 classes=None, crowd=None, num_classes=2, cls_specific=False):
    """One image: labels_int32 [n] and rois [n, 6] as the box-head sampler leaves them (fg rows first).  -> dict of masks int32
    [n_fg, Cm M^3], rois fp32 [n_fg, 6], assign int32 [n_fg], counts int64 [4] = fg rows, positive voxels, labelled voxels, 0."""
    labels_int32 = np.asarray(labels_int32).reshape(-1)
    fg = np.flatnonzero(labels_int32 > 0)
    rois_fg = np.asarray(rois, f32).reshape(-1, 6)[fg]
    boxes = spots_to_boxes(spots, in_size) if spots is not None else np.asarray(gt_boxes, f32).reshape(-1, 6)
    a = assign(rois_fg, boxes, classes, crowd)
    masks = np.zeros((len(fg), M ** 3), np.int32)
    for i, k in enumerate(a):
        if k < 0:
            continue
        if spots is not None:
            fn = spot_mask_closed if form == "closed" else spot_mask_direct
            masks[i] = fn(np.asarray(spots, f32).reshape(-1, 4)[k], rois_fg[i], M).reshape(-1)
        else:
            fn = label_mask_closed if form == "closed" else label_mask_direct
            masks[i] = fn(label_volume, int(np.asarray(markers)[k]), boxes[k], rois_fg[i], M).reshape(-1)
    if cls_specific:
        masks = expand(masks, labels_int32[fg], num_classes, M)
    counts = np.array([len(fg), int((masks == 1).sum()), int((masks > -1).sum()), 0], np.int64)
    return dict(masks=masks, rois=rois_fg, assign=a, counts=counts)


# ---------------------------------------------------------------- loss
def loss(x, t, weight=1.0, dtype=f64):
    """mask_rcnn_losses (mask_rcnn_heads.py:90-99): weight * sum over t > -1 of (max(x, 0) - x t + log1p(exp(-|x|))) / W and its gradient
    weight * (sigmoid(x) - t) / W at t > -1, 0 elsewhere; W = 0 gives 0 and zeros.  -> loss, grad (x's shape), W, sum |term|"""
    x = np.asarray(x)
    xs, ts = x.reshape(-1).astype(dtype), np.asarray(t).reshape(-1)
    on = ts > -1
    W = int(on.sum())
    g = np.zeros(xs.shape, dtype)
    if W == 0:
        return dtype(0), g.reshape(x.shape), 0, dtype(0)
    xv, tv = xs[on], ts[on].astype(dtype)
    term = np.maximum(xv, 0) - xv * tv + np.log1p(np.exp(-np.abs(xv)))
    e = np.exp(-np.abs(xv))
    sig = np.where(xv >= 0, 1 / (1 + e), e / (1 + e))
    g[on] = dtype(weight) * (sig - tv) / dtype(W)
    return dtype(weight) * term.sum(dtype=dtype) / dtype(W), g.reshape(x.shape), W, np.abs(term).sum(dtype=dtype)


def loss_bounds(l64, g64, W, abs_sum, weight, n):
    """How far an fp32 result may lie from the fp64 evaluation `l64, g64` of the same formulas on the same fp32 inputs.
    device: every term is a handful of fp64 operations (8 roundings, exp and log1p good to an ulp), the W terms are added in fp64 (at
    most W 2^-53 sum |term| whatever the order), then one divide, one product and one rounding to fp32: (W + 16) 2^-53 weight sum|term|
    / W + 2^-24 |loss|.  A gradient element: 8 fp64 roundings of a value <= weight / W, then one fp32 rounding.
    reference: torch sums n fp32 products (weight 0 at ignored elements) of fp32 terms, each good to a few ulp, in fp32 in an order of
    its own: gamma_n sum |term| / W with gamma_n = n 2^-24 / (1 - n 2^-24), plus 8 2^-24 for the terms and the two scalings.  Its
    gradient: a sigmoid <= 1 good to a few ulp, one subtraction (which may cancel), a product and a divide: 8 2^-24 of max(|g|,
    weight / W)."""
    if W == 0:
        return 0.0, 0.0, np.zeros_like(g64), np.zeros_like(g64)
    mean_abs = abs(weight) * float(abs_sum) / W
    dev_loss = (W + 16) * EPS64 * mean_abs + EPS32 * abs(float(l64))
    gam = n * EPS32 / (1 - n * EPS32)
    ref_loss = (gam + 8 * EPS32) * mean_abs
    floor = abs(weight) / W
    dev_grad = 8 * EPS64 * floor + EPS32 * np.abs(g64)
    ref_grad = 8 * EPS32 * np.maximum(np.abs(g64), floor)
    return dev_loss, ref_loss, dev_grad, ref_grad
