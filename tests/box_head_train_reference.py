"""NumPy restatement of the box-head training step (the checker of tests/test_box_head_train_host.py and
tests/test_gpu_box_head_train.py): proposal labelling, the seeded fg / bg sampling, regression targets, the dense blobs and the two
losses with their gradients.  Written from the description in DESIGN ("Box-head training targets");
tests/golden/gen_box_head_train.py checks it against the reference's own add_proposals / _sample_rois / fast_rcnn_losses.

"roidb rows" of an image: r = 0 .. K-1 its ground-truth boxes in the given order, then r = K .. its proposals in order."""
import numpy as np

from rpn_train_reference import key, overlaps, stream

f32, f64 = np.float32, np.float64
U = np.uint64


def make_cfg(batch=64, fg_fraction=0.25, fg_thresh=0.4, bg_hi=0.4, bg_lo=0.0, num_classes=2, weights=(10., 10., 10., 5., 5., 5.)):
    return dict(batch=int(batch), fg_fraction=float(fg_fraction), fg_thresh=float(fg_thresh), bg_hi=float(bg_hi), bg_lo=float(bg_lo),
                num_classes=int(num_classes), weights=tuple(float(w) for w in weights))


def fg_per_im(cfg):
    return int(np.round(cfg["fg_fraction"] * cfg["batch"]))


def label(gt, proposals, classes=None, crowd=None):
    """Everything that does not depend on the seed: per roidb row the box, the maximum overlap (fp32), the class and the assigned
    ground-truth row (-1 = none)."""
    gt = np.asarray(gt, f32).reshape(-1, 6)
    pr = np.asarray(proposals, f32).reshape(-1, 6)
    K, n = len(gt), len(pr)
    classes = np.ones(K, np.int32) if classes is None else np.asarray(classes, np.int32).reshape(K)
    crowd = np.zeros(K, bool) if crowd is None else np.asarray(crowd).astype(bool).reshape(K)
    ov = np.zeros(K + n, f32)
    cls = np.zeros(K + n, np.int32)
    assign = np.full(K + n, -1, np.int64)
    ov[:K] = np.where(crowd, f32(-1), f32(1))
    cls[:K] = np.where(crowd, 0, classes)
    assign[:K] = np.arange(K)              # box_to_gt_ind_map of a gt row is the row itself, crowd or not
    real = np.flatnonzero(~crowd)
    if len(real) and n:
        m = overlaps(pr, gt[real])
        arg = m.argmax(1)                      # the first maximum
        mx = m[np.arange(n), arg]
        hit = mx > 0
        ov[K:] = np.where(hit, mx, f32(0))
        cls[K:] = np.where(hit, classes[real[arg]], 0)
        assign[K:] = np.where(hit, real[arg], -1)
    return dict(K=K, n=n, boxes=np.concatenate([gt, pr], 0), gt=gt, overlap=ov, cls=cls, assign=assign, crowd=crowd)


def candidates(L, cfg):
    ov = L["overlap"]
    return np.flatnonzero(ov >= f32(cfg["fg_thresh"])), np.flatnonzero((ov < f32(cfg["bg_hi"])) & (ov >= f32(cfg["bg_lo"])))


def choose(cand, want, st, base):
    """the `want` candidates with the smallest (key(base + r), r), ascending in r"""
    k = key(st, cand.astype(U) + U(base))
    return np.sort(cand[np.lexsort((cand, k))[:want]])


def targets_of(b, q, weights):
    """bbox_transform_inv_3d on fp32 boxes: dx,dy,dz in fp32 as (w * (g - e)) / size; dw,dh,ds = fp32(w * log in fp64 of the fp32 ratio)"""
    b, q = np.asarray(b, f32).reshape(-1, 6), np.asarray(q, f32).reshape(-1, 6)
    one, half = f32(1.0), f32(0.5)
    e = [(b[:, 3 + d] - b[:, d]) + one for d in range(3)]
    g = [(q[:, 3 + d] - q[:, d]) + one for d in range(3)]
    ec = [b[:, d] + half * e[d] for d in range(3)]
    gc = [q[:, d] + half * g[d] for d in range(3)]
    cols = [(f32(weights[d]) * (gc[d] - ec[d])) / e[d] for d in range(3)]
    cols += [(f64(weights[3 + d]) * np.log((g[d] / e[d]).astype(f64))).astype(f32) for d in range(3)]
    return np.stack(cols, 1).astype(f32)


def sample(L, cfg, seed):
    """The seeded part: rows, labels, rois, compact targets, counts (trimmed to the number of rows sampled)."""
    st = stream(seed)
    fgc, bgc = candidates(L, cfg)
    fg = choose(fgc, min(fg_per_im(cfg), len(fgc)), st, 0)
    bg = choose(bgc, min(cfg["batch"] - len(fg), len(bgc)), st, 1 << 40)
    rows = np.concatenate([fg, bg]).astype(np.int64)
    labels = np.concatenate([L["cls"][fg], np.zeros(len(bg), np.int32)]).astype(np.int32)
    rois = L["boxes"][rows]
    tg = np.zeros((len(rows), 6), f32)
    on = np.flatnonzero(labels > 0)
    tg[on] = targets_of(rois[on], L["gt"][L["assign"][rows[on]]], cfg["weights"])
    counts = np.array([len(rows), len(fg), len(bg), len(fgc), len(bgc), int(L["crowd"].sum()), L["K"] - int(L["crowd"].sum()), L["n"]],
                      np.int64)
    return dict(rows=rows, labels=labels, rois=rois.astype(f32), targets=tg, counts=counts)


def box_head_targets(gt, proposals, cfg, seed, classes=None, crowd=None):
    return sample(label(gt, proposals, classes, crowd), cfg, seed)


def blobs(T, cfg):
    """bbox_targets, bbox_inside_weights, bbox_outside_weights fp32 [rows, 6 C]"""
    C = cfg["num_classes"]
    n = len(T["labels"])
    bt, iw = np.zeros((n, 6 * C), f32), np.zeros((n, 6 * C), f32)
    for i in np.flatnonzero(T["labels"] > 0):
        c = int(T["labels"][i])
        bt[i, 6 * c:6 * c + 6] = T["targets"][i]
        iw[i, 6 * c:6 * c + 6] = 1
    return bt, iw, (iw > 0).astype(f32)


def losses(score, pred, labels, targets, dtype=f64):
    """loss_cls, loss_bbox, accuracy_cls, d loss_cls / d score, d loss_bbox / d pred, R of the softmax cross entropy and smooth L1
    (beta = 1) over the rows with label >= 0, evaluated in `dtype` on the given inputs.  score [N,C], pred [N,6C], labels [N] (-1 =
    padding), targets [N,6] compact."""
    score, pred, labels = np.asarray(score), np.asarray(pred), np.asarray(labels).reshape(-1)
    N, C = score.shape
    gs, gp = np.zeros(score.shape, dtype), np.zeros(pred.shape, dtype)
    rows = np.flatnonzero(labels >= 0)
    R = len(rows)
    if R == 0:
        return dtype(0), dtype(0), dtype(0), gs, gp, 0
    s = score[rows].astype(dtype)
    y = labels[rows].astype(np.int64)
    m = s.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(s - m).sum(1, dtype=dtype))
    lc = (lse - s[np.arange(R), y]).sum(dtype=dtype) / dtype(R)
    acc = dtype((score[rows].argmax(1) == y).sum()) / dtype(R)
    sm = np.exp(s - lse[:, None])
    sm[np.arange(R), y] -= dtype(1)
    gs[rows] = sm / dtype(R)
    lb = dtype(0)
    fg = rows[y > 0]
    if len(fg):
        slot = 6 * labels[fg].astype(np.int64)[:, None] + np.arange(6)[None, :]
        d = pred[fg[:, None], slot].astype(dtype) - np.asarray(targets)[fg].astype(dtype)
        ad = np.abs(d)
        lb = np.where(ad < 1, dtype(0.5) * d * d, ad - dtype(0.5)).sum(dtype=dtype) / dtype(R)
        gp[fg[:, None], slot] = np.clip(d, -1, 1) / dtype(R)
    return lc, lb, acc, gs, gp, R
