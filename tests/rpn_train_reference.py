"""NumPy restatement of the RPN training step (the checker of tests/test_rpn_train_host.py and tests/test_gpu_rpn_train.py): anchor
labelling over the wide field, the seeded sampling contract, regression targets, the dense "wide" blobs and the two losses with their
gradients.  Written from the description in DESIGN ("RPN training targets"); tests/golden/gen_rpn_train.py checks it against the
reference's own _get_rpn_blobs / single_scale_rpn_losses.

Index conventions: "field index" i = position * A + a with position = (z F + y) F + x; "wide index" = a F^3 + position (the
[A, F, F, F] blob)."""
import numpy as np

from m3d.config import generate_anchors_3d

f32, f64 = np.float32, np.float64
U = np.uint64


def key(seed, idx):
    """upper 32 bits of the splitmix64 finaliser of seed + idx (mod 2^64)"""
    with np.errstate(over="ignore"):
        z = (np.asarray(idx).astype(U) + U(int(seed) & (2 ** 64 - 1))) * U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z = z ^ (z >> U(31))
    return z >> U(32)


def stream(seed):
    """the sampling stream of a seed: the full 64-bit splitmix64 finaliser of the seed; keys are taken as key(stream(seed), i)"""
    with np.errstate(over="ignore"):
        z = U(int(seed) & (2 ** 64 - 1)) * U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        z = z ^ (z >> U(31))
    return int(z)


def make_cfg(stride, sizes, aspect_ratios, max_size, batch, positive, negative, straddle=0, fg_fraction=0.5, coarsest_stride=32):
    return dict(stride=int(stride), sizes=tuple(sizes), aspect_ratios=[list(map(float, r)) for r in aspect_ratios], max_size=int(max_size),
                batch=int(batch), positive=float(positive), negative=float(negative), straddle=float(straddle),
                fg_fraction=float(fg_fraction), coarsest_stride=int(coarsest_stride))


def field_size(cfg):
    m = cfg["coarsest_stride"] * np.ceil(cfg["max_size"] / float(cfg["coarsest_stride"]))
    return int(np.ceil(m / float(cfg["stride"])))


def field_anchors(cfg):
    """fp32 [F^3 A, 6] in field order, A, F"""
    cell = generate_anchors_3d(cfg["stride"], cfg["sizes"], cfg["aspect_ratios"])
    F = field_size(cfg)
    s = np.arange(F, dtype=np.int64) * cfg["stride"]
    z, y, x = np.meshgrid(s, s, s, indexing="ij")
    sh = np.stack([x.ravel(), y.ravel(), z.ravel()] * 2, 1).astype(f64)
    return (cell[None, :, :] + sh[:, None, :]).reshape(-1, 6).astype(f32), cell.shape[0], F


def overlaps(b, q, rows=32768):
    """IoU matrix fp32 [n, K]: fp32 intersection, fp64 union and divide, fp32 store; exactly 0 without intersection"""
    b, q = np.ascontiguousarray(b, f32), np.ascontiguousarray(q, f32).reshape(-1, 6)
    out = np.zeros((len(b), len(q)), f32)
    if not len(q):
        return out
    qv = ((((q[:, 3] - q[:, 0]).astype(f64) + 1.0) * ((q[:, 4] - q[:, 1]).astype(f64) + 1.0)) * ((q[:, 5] - q[:, 2]).astype(f64) + 1.0)).astype(f32)
    for lo in range(0, len(b), rows):
        c = b[lo:lo + rows]
        ext = [((np.minimum(c[:, None, 3 + d], q[None, :, 3 + d]) - np.maximum(c[:, None, d], q[None, :, d])).astype(f64) + 1.0).astype(f32)
               for d in range(3)]
        hit = (ext[0] > 0) & (ext[1] > 0) & (ext[2] > 0)
        inter = (ext[0] * ext[1]) * ext[2]
        bv = (((c[:, 3] - c[:, 0]).astype(f64) + 1.0) * ((c[:, 4] - c[:, 1]).astype(f64) + 1.0)) * ((c[:, 5] - c[:, 2]).astype(f64) + 1.0)
        uv = (bv[:, None] + qv.astype(f64)[None, :]) - inter.astype(f64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = (inter.astype(f64) / uv).astype(f32)
        out[lo:lo + rows] = np.where(hit, r, f32(0))
    return out


def label(gt, dc, im_size, cfg):
    """Everything that does not depend on the seed.  im_size = (slices, height, width)."""
    gt = np.asarray(gt, f32).reshape(-1, 6)
    dc = np.zeros((0, 6), f32) if dc is None else np.asarray(dc, f32).reshape(-1, 6)
    an, A, F = field_anchors(cfg)
    S, H, W = [float(v) for v in im_size]
    t = cfg["straddle"]
    if t >= 0:
        inside = np.where((an[:, 0] >= -t) & (an[:, 1] >= -t) & (an[:, 2] >= -t) & (an[:, 3] < W + t) & (an[:, 4] < H + t) & (an[:, 5] < S + t))[0]
    else:
        inside = np.arange(len(an))
    a = an[inside]
    n = len(inside)
    mx, arg, fg = np.zeros(n, f32), np.zeros(n, np.int64), np.zeros(n, bool)
    if len(gt):
        gmax = np.zeros(len(gt), f32)
        step = 32768
        for lo in range(0, n, step):
            ov = overlaps(a[lo:lo + step], gt)
            gmax = np.maximum(gmax, ov.max(0)) if len(ov) else gmax
            arg[lo:lo + step] = ov.argmax(1)
            mx[lo:lo + step] = ov.max(1)
        for lo in range(0, n, step):
            ov = overlaps(a[lo:lo + step], gt)
            fg[lo:lo + step] = (ov == gmax[None, :]).any(1)
        fg |= mx >= f32(cfg["positive"])
    dmx = overlaps(a, dc).max(1) if len(dc) else np.zeros(n, f32)
    cand = (mx < f32(cfg["negative"])) & (dmx < f32(cfg["negative"]))
    return dict(A=A, F=F, N=len(an), inside=inside, anchors=a, gt=gt, mx=mx, arg=arg, fg=fg, cand=cand)


def wide_index(L, field_idx):
    field_idx = np.asarray(field_idx, np.int64)
    return (field_idx % L["A"]) * L["F"] ** 3 + field_idx // L["A"]


def targets_of(b, q):
    """bbox_transform_inv_3d with unit weights in fp32; the three logs in fp64, rounded once"""
    b, q = np.asarray(b, f32), np.asarray(q, f32)
    one, half = f32(1.0), f32(0.5)
    e = [(b[:, 3 + d] - b[:, d]) + one for d in range(3)]
    g = [(q[:, 3 + d] - q[:, d]) + one for d in range(3)]
    ec = [b[:, d] + half * e[d] for d in range(3)]
    gc = [q[:, d] + half * g[d] for d in range(3)]
    cols = [(gc[d] - ec[d]) / e[d] for d in range(3)] + [np.log((g[d] / e[d]).astype(f64)).astype(f32) for d in range(3)]
    return np.stack(cols, 1).astype(f32) if len(b) else np.zeros((0, 6), f32)


def sample(L, cfg, seed):
    """The seeded part: fg subsampling, bg draws, targets, counts."""
    inside = L["inside"]
    seed = stream(seed)
    batch = cfg["batch"]
    num_fg = int(cfg["fg_fraction"] * batch)
    fg_rel = np.where(L["fg"])[0]
    fg_before = len(fg_rel)
    if fg_before > num_fg:
        fld = inside[fg_rel]
        order = np.lexsort((fld, key(seed, fld)))
        fg_rel = np.sort(fg_rel[order[:num_fg]])
    lab = np.full(len(inside), -1, np.int32)
    lab[fg_rel] = 1
    cand_rel = np.where(L["cand"])[0]
    n = len(cand_rel)
    num_bg = batch - len(fg_rel)
    draws = 0
    if n > num_bg:
        draws = num_bg
        r = (key(seed, np.arange(num_bg, dtype=U) + U(1 << 40)) * U(n)) >> U(32)
        lab[cand_rel[r.astype(np.int64)]] = 0
    num_examples = int((lab >= 0).sum())
    tw = wide_index(L, inside[fg_rel])
    o = np.argsort(tw, kind="stable")
    fgw = wide_index(L, inside[lab == 1])
    bgw = wide_index(L, inside[lab == 0])
    return dict(A=L["A"], F=L["F"], fg_index=np.sort(fgw), bg_index=np.sort(bgw), target_index=tw[o],
                targets=targets_of(L["anchors"][fg_rel], L["gt"][L["arg"][fg_rel]])[o], num_examples=num_examples,
                counts=np.array([len(fgw), len(bgw), len(fg_rel), num_examples, len(inside), fg_before, n, draws], np.int64))


def rpn_targets(gt, im_size, cfg, seed, dc=None):
    return sample(label(gt, dc, im_size, cfg), cfg, seed)


def outside_weight(T):
    return f32(1.0 / T["num_examples"]) if T["num_examples"] else f32(0)


def wide(T):
    """labels int32 [1,A,F,F,F], targets / inside / outside weights fp32 [1,6A,F,F,F]"""
    A, F = T["A"], T["F"]
    F3 = F ** 3
    lab = np.full(A * F3, -1, np.int32)
    lab[T["fg_index"]] = 1
    lab[T["bg_index"]] = 0
    tg, iw, ow = (np.zeros((A, 6, F3), f32) for _ in range(3))
    tg[T["target_index"] // F3, :, T["target_index"] % F3] = T["targets"]
    iw[T["fg_index"] // F3, :, T["fg_index"] % F3] = 1
    for ix in (T["fg_index"], T["bg_index"]):
        ow[ix // F3, :, ix % F3] = outside_weight(T)
    shp = (1, 6 * A, F, F, F)
    return lab.reshape(1, A, F, F, F), tg.reshape(shp), iw.reshape(shp), ow.reshape(shp)


def losses(logits, pred, Ts, dtype=f64):
    """loss_cls, loss_bbox, d loss_cls / d logits, d loss_bbox / d pred, W (the sum of the classification weights) of the sigmoid RPN
    loss and smooth L1 with beta = 1/9 over the sampled anchors inside the crop [:s,:h,:w], evaluated in `dtype` on the given inputs."""
    logits, pred = np.asarray(logits), np.asarray(pred)
    B, A, s, h, w = logits.shape
    beta = dtype(1.0 / 9.0)
    gl, gp = np.zeros(logits.shape, dtype), np.zeros(pred.shape, dtype)
    items = []
    for b, T in enumerate(Ts):
        F = T["F"]
        F3 = F ** 3
        for idx, y in ((T["fg_index"], 1), (T["bg_index"], 0)):
            a, pos = idx // F3, idx % F3
            z, yy, x = pos // (F * F), (pos // F) % F, pos % F
            ok = (z < s) & (yy < h) & (x < w)
            items.append((b, T, y, idx[ok], a[ok], z[ok], yy[ok], x[ok]))
    W = sum(len(it[3]) for it in items)
    lc, lb = dtype(0), dtype(0)
    for b, T, y, idx, a, z, yy, x in items:
        xv = logits[b, a, z, yy, x].astype(dtype)
        lc += (np.maximum(xv, 0) - xv * y + np.log1p(np.exp(-np.abs(xv)))).sum(dtype=dtype)
        e = np.exp(-np.abs(xv))
        sig = np.where(xv >= 0, 1 / (1 + e), e / (1 + e))
        gl[b, a, z, yy, x] = (sig - y) / dtype(W)
        if y != 1 or not len(idx):
            continue
        row = np.searchsorted(T["target_index"], idx)
        assert np.array_equal(T["target_index"][row], idx)
        o = dtype(outside_weight(T))
        for d in range(6):
            v = pred[b, 6 * a + d, z, yy, x].astype(dtype) - T["targets"][row, d].astype(dtype)
            av = np.abs(v)
            lb += (o * np.where(av < beta, dtype(0.5) * v * v / beta, av - dtype(0.5) * beta)).sum(dtype=dtype)
            gp[b, 6 * a + d, z, yy, x] = o * np.clip(v / beta, -1, 1) / dtype(B)
    return (lc / dtype(W) if W else dtype(0)), lb / dtype(B), gl, gp, W
