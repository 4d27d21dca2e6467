"""NumPy restatement of the training-sample contract (DESIGN, "Training samples"): the annotation readers of the two datasets, the
key-drawn starts, the crop search, the crop, the box filter and the epoch order.  Independent of m3d/data.py and of the kernels: the
tests compare both with this file, and tests/golden/gen_train_sample.py compares this file with the reference's own functions.

Axis order: volumes and IN_SIZE are (slices, height, width); origins, starts and start_max are (x, y, z); boxes are fp32
(x1, y1, z1, x2, y2, z2)."""
import numpy as np

from rpn_train_reference import key, stream

f32, f64 = np.float32, np.float64
PI = 3.14159                          # the constant of both dataset classes


# ---------------------------------------------------------------- annotation readers
def _sanitise(objs, im_size):
    """_add_gt_annotations of both datasets: (x1,y1,z1,w,h,s) -> clipped corners; boxes with no volume or no extent on an axis are dropped"""
    S, H, W = im_size
    keep = []
    for o in objs:
        x1, y1, z1, w, h, s = o["bbox"]
        x2, y2, z2 = x1 + max(0.0, w - 1.0), y1 + max(0.0, h - 1.0), z1 + max(0.0, s - 1.0)
        x1, x2 = (min(W - 1.0, max(0.0, v)) for v in (x1, x2))
        y1, y2 = (min(H - 1.0, max(0.0, v)) for v in (y1, y2))
        z1, z2 = (min(S - 1.0, max(0.0, v)) for v in (z1, z2))
        if o["volume"] > 0 and x2 > x1 and y2 > y1 and z2 > z1:
            keep.append((o, [x1, y1, z1, x2, y2, z2]))
    boxes = np.array([b for _, b in keep], f32).reshape(-1, 6)
    classes = np.ones(len(keep), np.int32)
    crowd = np.array([o["iscrowd"] for o, _ in keep], bool)
    volumes = np.array([o["volume"] for o, _ in keep], f32)
    return boxes, classes, crowd, volumes, [o for o, _ in keep]


def read_soma(lines, im_size, radius_exp_ratio):
    """soma_dataset.py:197-289 on the lines of an annotation file (the first is a header) -> boxes, classes, crowd, segms [K,4], volumes"""
    S, H, W = im_size
    objs = []
    for a in lines[1:]:
        p = a.rstrip().split(" ")
        px, py, pz = min(W - 1, int(p[0])), min(H - 1, int(p[1])), min(S - 1, int(p[2]))
        r = int(p[3])
        d = r * 2 * (1.0 + radius_exp_ratio)
        x1, y1, z1 = int(max(px - d / 2.0, 0.0)), int(max(py - d / 2.0, 0.0)), int(max(pz - d / 2.0, 0.0))
        w = int(min(px + d / 2.0, W - 1)) - x1 + 1
        h = int(min(py + d / 2.0, H - 1)) - y1 + 1
        s = int(min(pz + d / 2.0, S - 1)) - z1 + 1
        objs.append(dict(bbox=[x1, y1, z1, w, h, s], seg=[px, py, pz, r], volume=4.0 / 3.0 * PI * r ** 3, iscrowd=0))
    boxes, classes, crowd, volumes, kept = _sanitise(objs, im_size)
    return boxes, classes, crowd, np.array([o["seg"] for o in kept], f32).reshape(-1, 4), volumes


def read_nuclei(lines, mask, im_size):
    """nuclei_dataset.py:214-252 and its _add_gt_annotations -> boxes, classes, crowd, volumes (voxels of the marker inside the box)"""
    S, H, W = im_size
    ann = lines[1:]
    objs, valid = [], False
    for a in ann:
        p = a.rstrip().split(" ")
        x1, y1, z1 = min(W - 1, int(float(p[1]))), min(H - 1, int(float(p[2]))), min(S - 1, int(float(p[3])))
        w, h, s, marker = int(float(p[4])), int(float(p[5])), int(float(p[6])), int(p[7])
        vol = int(np.sum(mask[z1:z1 + s, y1:y1 + h, x1:x1 + w] == marker))
        c1 = (x1 == 0 or x1 + w - 1 >= W) and w < 25
        c2 = (y1 == 0 or y1 + h - 1 >= H) and h < 25
        c3 = valid or a != ann[-1]                      # the "last line" condition: a comparison of the lines' text
        crowd = int((c1 or c2) and c3)
        if not crowd:
            valid = True
        objs.append(dict(bbox=[x1, y1, z1, w, h, s], volume=vol, iscrowd=crowd))
    return _sanitise(objs, im_size)[:4]


# ---------------------------------------------------------------- the crop
def start_max(boxes, dims, in_size):
    """(x, y, z): min(floor(min lower coordinate), dim - size), blob.py:106-114"""
    D, H, W = dims
    s, h, w = in_size
    b = np.asarray(boxes, f32).reshape(-1, 6)
    return tuple(int(min(int(np.floor(b[:, a].min())), d - n)) for a, d, n in ((0, W, w), (1, H, h), (2, D, s)))


def draw_starts(seed, smax):
    """the sampling contract standing in for npr.choice(range(0, start_max + 1)): 0 where start_max == 0, no draw"""
    st = stream(seed)
    return tuple(0 if m == 0 else int((int(key(st, a)) * (m + 1)) >> 32) for a, m in enumerate(smax))


def axis_list(start, dim, size):
    return list(range(start, dim - size, size // 2)) + [dim - size]


def shift_clip(boxes, origin, in_size):
    """fp32 clip(b - o, 0, size - 1) and the rows it leaves non-degenerate"""
    s, h, w = in_size
    b = np.array(boxes, f32).reshape(-1, 6)
    for a, n in ((0, w), (1, h), (2, s)):
        b[:, a::3] = np.minimum(np.maximum(b[:, a::3] - f32(origin[a]), f32(0)), f32(n - 1))
    ok = ~((b[:, 0] == b[:, 3]) | (b[:, 1] == b[:, 4]) | (b[:, 2] == b[:, 5]))
    return b, ok


def score_of(boxes, origin, in_size):
    """the clipped box volume a candidate contains: fp64, added in box order"""
    b, ok = shift_clip(boxes, origin, in_size)
    b = b.astype(f64)
    total = 0.0
    for k in np.flatnonzero(ok):
        total += (((b[k, 3] - b[k, 0]) + 1.0) * ((b[k, 4] - b[k, 1]) + 1.0)) * ((b[k, 5] - b[k, 2]) + 1.0)
    return total


def candidates(starts, dims, in_size):
    """origins (x, y, z) in the order of the search: z outer, y, x inner"""
    D, H, W = dims
    s, h, w = in_size
    xs, ys, zs = axis_list(starts[0], W, w), axis_list(starts[1], H, h), axis_list(starts[2], D, s)
    return [(x, y, z) for z in zs for y in ys for x in xs]


def search(boxes, cands, in_size):
    """first strict maximum -> (origin, score, status, all scores); status 1: nothing above 0, the first candidate"""
    scores = [score_of(boxes, o, in_size) for o in cands]
    best, at = 0.0, -1
    for i, v in enumerate(scores):
        if v > best:
            best, at = v, i
    return cands[max(at, 0)], best, int(at < 0), scores


def sample(boxes, dims, in_size, seed, need_crop=True, fixed_origin=None, max_boxes=None):
    """What m3d_train_sample writes for one image: dict(info int32 [8], boxes [max_boxes,6], keep int32 [max_boxes], score, origin)"""
    boxes = np.asarray(boxes, f32).reshape(-1, 6)
    K = len(boxes)
    M = K if max_boxes is None else max_boxes
    if not need_crop:
        origin, best, status, ncand, kept, idx = (0, 0, 0), 0.0, 0, 0, boxes.copy(), np.arange(K)
    else:
        if fixed_origin is not None:
            cands = [tuple(int(v) for v in fixed_origin)]
        else:
            cands = candidates(draw_starts(seed, start_max(boxes, dims, in_size)), dims, in_size)
        origin, best, status, _ = search(boxes, cands, in_size)
        ncand = len(cands)
        b, ok = shift_clip(boxes, origin, in_size)
        idx = np.flatnonzero(ok)
        kept = b[idx]
    out_b, out_k = np.zeros((M, 6), f32), np.full((M,), -1, np.int32)
    out_b[:len(idx)], out_k[:len(idx)] = kept, idx
    info = np.array([origin[0], origin[1], origin[2], len(idx), status, ncand, 0, 0], np.int32)
    return dict(info=info, boxes=out_b, keep=out_k, score=f64(best), origin=origin)


def crop(vol, origin, in_size):
    x, y, z = origin
    s, h, w = in_size
    return vol[z:z + s, y:y + h, x:x + w]


# ---------------------------------------------------------------- the order of an epoch
ORDER_BASE = 1 << 40


def epoch_order(n, seed, epoch):
    """MinibatchSampler without aspect grouping: a permutation of range(n) per epoch, here the indices in ascending
    (key(stream(seed), 2^40 + epoch n + i), i)"""
    i = np.arange(n, dtype=np.uint64)
    k = key(stream(seed), i + np.uint64(ORDER_BASE + epoch * n))
    return np.lexsort((i, k)).astype(np.int64)


def batch_indices(n, ims_per_batch, steps, seed):
    """the image indices of `steps` minibatches: whole batches of every epoch's order (BatchSampler with drop_last)"""
    out, epoch = [], 0
    while len(out) < steps:
        o = epoch_order(n, seed, epoch)
        for j in range(n // ims_per_batch):
            out.append([int(v) for v in o[j * ims_per_batch:(j + 1) * ims_per_batch]])
        epoch += 1
    return out[:steps]


def batch_seeds(seed, step, ims_per_batch):
    """the per-image seeds of minibatch `step`"""
    return [int(seed) + 1 + step * ims_per_batch + b for b in range(ims_per_batch)]
