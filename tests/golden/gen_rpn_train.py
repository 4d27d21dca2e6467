"""Golden vectors for the RPN training step: runs the REFERENCE's own `roi_data.rpn._get_rpn_blobs` and
`modeling.rpn_heads.single_scale_rpn_losses` (+ autograd) on the CPU through oracle/ref_harness.py and writes tests/golden/rpn_train.npz.

`roi_data.rpn.npr` is replaced by an object whose `choice` / `randint` implement the sampling contract of DESIGN ("RPN training
targets"): keys are taken in the seed's stream (`stream(seed)`) on the flat FIELD index, so the inside-relative indices the reference hands over are mapped back through the
same inside test.  `data_utils._threadlocal_foa.cache` is cleared between cases: its key ignores TRAIN.MAX_SIZE.

The generator asserts the properties the cases exist for (fg subsampling, both fg rules, duplicate draws, draws outside the crop, a
fg -> bg flip, don't-care boxes, no bg at all), so a later edit of the inputs cannot silently drop one.

Run in the build container only:  python tests/golden/gen_rpn_train.py"""
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import rpn_train_reference as R  # noqa: E402

NUC = "configs/cell_tracking_baseline/e2e_mask_rcnn_N3DH_SIM_dsn_body.yaml"
SOMA = "configs/soma_starting/e2e_mask_rcnn_soma_dsn_body.yaml"
SMALL = ("TRAIN.MAX_SIZE", 64, "TRAIN.IN_SIZE", (32, 64, 48))
# name, yaml, overrides, boxes, seed, special, dense blobs in the file
CASES = [
    ("nuclei", NUC, (), 40, 1, None, False),
    ("soma", SOMA, (), 60, 2, None, False),
    ("small_all", NUC, SMALL + ("TRAIN.RPN_STRADDLE_THRESH", -1, "TRAIN.RPN_BATCH_SIZE_PER_IM", 4096), 6, 3, None, True),
    ("small_outside", NUC, SMALL + ("TRAIN.RPN_STRADDLE_THRESH", 0, "TRAIN.RPN_BATCH_SIZE_PER_IM", 64), 6, 4, "outside_gt", True),
    ("small_dc", NUC, SMALL + ("TRAIN.RPN_STRADDLE_THRESH", 0, "TRAIN.RPN_BATCH_SIZE_PER_IM", 64), 6, 5, "dc", True),
    ("small_nobg", NUC, SMALL + ("TRAIN.RPN_STRADDLE_THRESH", 0, "TRAIN.RPN_BATCH_SIZE_PER_IM", 4096), 6, 6, None, True),
]
LOSS_CASES = [("loss_nuclei", ["nuclei"], 11), ("loss_soma", ["soma"], 12), ("loss_small2", ["small_all", "small_outside"], 13)]


def make_boxes(seed, K, S, H, W):
    rng = np.random.RandomState(seed)
    c = np.stack([rng.uniform(8, W - 8, K), rng.uniform(8, H - 8, K), rng.uniform(6, S - 6, K)], 1)
    r = rng.uniform(4, 12, (K, 3))
    return np.round(np.concatenate([c - r, c + r], 1)).astype(np.float32)


def loss_inputs(seed, B, A, s, h, w):
    rng = np.random.RandomState(seed)
    return ((rng.standard_normal((B, A, s, h, w)) * 2).astype(np.float32), (rng.standard_normal((B, 6 * A, s, h, w)) * 0.5).astype(np.float32))


class FakeNpr:
    def __init__(self, seed, inside):
        self.seed, self.inside, self.log = R.stream(seed), inside, {"fg_before": None, "bg_cand": None, "draws": 0, "distinct": 0}

    def choice(self, a, size, replace):
        assert replace is False
        order = np.lexsort((self.inside[a], R.key(self.seed, self.inside[a])))   # ascending (key, field index)
        self.log["fg_before"] = len(a)
        return a[order[len(a) - size:]]                                          # disabled: all but the num_fg smallest

    def randint(self, n, size):
        j = np.arange(size, dtype=np.uint64) + np.uint64(1 << 40)
        r = (R.key(self.seed, j) * np.uint64(n)) >> np.uint64(32)
        self.log.update(bg_cand=n, draws=int(size), distinct=len(np.unique(r)))
        return r.astype(np.int64)


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def run_case(H, yml, overrides, K, seed, special):
    import roi_data.data_utils as DU
    import roi_data.rpn as RPN
    cfg = H.load_cfg(yml, overrides)
    if hasattr(DU._threadlocal_foa, "cache"):
        DU._threadlocal_foa.cache.clear()
    foa = DU.get_field_of_anchors(cfg.RPN.STRIDE, cfg.RPN.SIZES, cfg.RPN.ASPECT_RATIOS)
    S, Hh, W = cfg.TRAIN.IN_SIZE
    gt = make_boxes(seed, K, S, Hh, W)
    dc = np.zeros((0, 6), np.float32)
    if special == "outside_gt":
        gt[0] = [W + 50, Hh + 50, S + 50, W + 60, Hh + 60, S + 60]
    if special == "dc":
        dc = np.array([[0, 0, 0, 23, 31, 15], [20, 30, 10, 40, 50, 30]], np.float32)
    an, t = foa.field_of_anchors, cfg.TRAIN.RPN_STRADDLE_THRESH
    inside = (np.where((an[:, 0] >= -t) & (an[:, 1] >= -t) & (an[:, 2] >= -t) & (an[:, 3] < W + t) & (an[:, 4] < Hh + t) & (an[:, 5] < S + t))[0]
              if t >= 0 else np.arange(len(an)))
    fake = FakeNpr(seed, inside)
    RPN.npr = fake
    blobs = RPN._get_rpn_blobs(float(S), float(Hh), float(W), [foa], an, gt, dc)
    rc = R.make_cfg(cfg.RPN.STRIDE, cfg.RPN.SIZES, cfg.RPN.ASPECT_RATIOS, cfg.TRAIN.MAX_SIZE, cfg.TRAIN.RPN_BATCH_SIZE_PER_IM,
                    cfg.TRAIN.RPN_POSITIVE_OVERLAP, cfg.TRAIN.RPN_NEGATIVE_OVERLAP, t, cfg.TRAIN.RPN_FG_FRACTION, cfg.FPN.COARSEST_STRIDE)
    assert foa.field_size == R.field_size(rc) and np.array_equal(an, R.field_anchors(rc)[0])
    return dict(cfg=rc, gt=gt, dc=dc, im_size=(S, Hh, W), seed=seed, blobs=blobs, log=fake.log, inside=len(inside), A=foa.num_cell_anchors,
                F=foa.field_size)


def sparse_of(c):
    """the reference's dense blobs -> the sparse sets (wide indices, ascending)"""
    A, F = c["A"], c["F"]
    lab = c["blobs"]["rpn_labels_int32_wide"].reshape(-1)
    tg = c["blobs"]["rpn_bbox_targets_wide"].reshape(A, 6, F ** 3)
    has = (tg != 0).any(1)
    a, pos = np.nonzero(has)
    tix = a.astype(np.int64) * F ** 3 + pos
    return np.flatnonzero(lab == 1), np.flatnonzero(lab == 0), tix, tg[a, :, pos].astype(np.float32)


def build_arrays():
    import ref_harness as H
    H.install()
    import torch
    import modeling.rpn_heads as RH
    out, cases = {}, {}
    for name, yml, ov, K, seed, special, dense in CASES:
        c = cases[name] = run_case(H, yml, ov, K, seed, special)
        fg, bg, tix, trows = sparse_of(c)
        b, rc, log = c["blobs"], c["cfg"], c["log"]
        num_fg = int(rc["fg_fraction"] * rc["batch"])
        fg_before = log["fg_before"] if log["fg_before"] is not None else len(tix)
        assert len(tix) == min(fg_before, num_fg), "a target row of zeros hides a sampled fg anchor: pick another seed"
        num_examples = len(fg) + len(bg)
        ow = b["rpn_bbox_outside_weights_wide"]
        assert num_examples == 0 or np.all(ow[ow != 0] == np.float32(1.0 / num_examples))
        c.update(fg=fg, bg=bg, tix=tix, trows=trows, num_examples=num_examples, fg_before=fg_before)
        p = name + "_"
        out[p + "gt"], out[p + "dc"] = c["gt"], c["dc"]
        out[p + "im_size"] = np.array(c["im_size"], np.int64)
        out[p + "seed"] = np.array(seed, np.int64)
        out[p + "sizes"] = np.array(rc["sizes"], np.float64)
        out[p + "aspect_ratios"] = np.array(rc["aspect_ratios"], np.float64)
        out[p + "numbers"] = np.array([rc["stride"], rc["max_size"], rc["batch"], rc["positive"], rc["negative"], rc["straddle"],
                                       rc["fg_fraction"], rc["coarsest_stride"]], np.float64)
        out[p + "fg_index"], out[p + "bg_index"], out[p + "target_index"], out[p + "targets"] = fg, bg, tix, trows
        out[p + "counts"] = np.array([len(fg), len(bg), len(tix), num_examples, c["inside"], fg_before,
                                      -1 if log["bg_cand"] is None else log["bg_cand"], log["draws"]], np.int64)
        out[p + "sha_labels"] = sha(b["rpn_labels_int32_wide"].astype(np.int32))
        out[p + "sha_inside"] = sha(b["rpn_bbox_inside_weights_wide"].astype(np.float32))
        out[p + "sha_outside"] = sha(b["rpn_bbox_outside_weights_wide"].astype(np.float32))
        if dense:
            out[p + "labels_wide"] = np.ascontiguousarray(b["rpn_labels_int32_wide"], np.int32)
            out[p + "targets_wide"] = np.ascontiguousarray(b["rpn_bbox_targets_wide"], np.float32)
            out[p + "inside_wide"] = np.ascontiguousarray(b["rpn_bbox_inside_weights_wide"], np.float32)
            out[p + "outside_wide"] = np.ascontiguousarray(b["rpn_bbox_outside_weights_wide"], np.float32)
        print(name, "inside", c["inside"], "fg before", fg_before, "fg", len(fg), "bg", len(bg), log)

    # ---- the properties the cases exist for
    def below(c):   # sampled fg anchors that only the tie rule made fg
        L = R.label(c["gt"], c["dc"], c["im_size"], c["cfg"])
        w = R.wide_index(L, L["inside"])
        return int((L["mx"][np.isin(w, c["tix"])] < np.float32(c["cfg"]["positive"])).sum())

    n, s, sa, so, sd, sn = (cases[k] for k in ("nuclei", "soma", "small_all", "small_outside", "small_dc", "small_nobg"))
    assert n["fg_before"] > 32 and len(n["tix"]) == 32 and below(n) == 32, "nuclei: fg subsampling, all by the tie rule"
    assert s["fg_before"] > 64 and len(s["tix"]) == 64 and below(s) == 0, "soma: fg subsampling, all by the threshold rule"
    assert sa["log"]["distinct"] < sa["log"]["draws"], "duplicate draws"
    F = sa["F"]
    pos = sa["bg"] % F ** 3
    st = sa["cfg"]["stride"]
    crop = [v // st for v in sa["im_size"]]
    outside_crop = (pos // (F * F) >= crop[0]) | ((pos // F) % F >= crop[1]) | (pos % F >= crop[2])
    assert outside_crop.sum() > 0, "bg draws outside the crop"
    assert so["fg_before"] == so["inside"] and len(so["fg"]) < len(so["tix"]), "a gt box outside the image; fg -> bg flips"
    assert sd["dc"].size and sd["log"]["bg_cand"] < R.label(sd["gt"], None, sd["im_size"], sd["cfg"])["cand"].sum(), "don't-care boxes"
    assert sn["log"]["bg_cand"] is None and len(sn["bg"]) == 0, "n <= num_bg: no bg at all"

    # ---- losses and gradients of the reference (fp32 torch + autograd) for seeded logits / predictions
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # torch's fp32 sum over the dense blobs depends on how many threads split it
    for lname, names, lseed in LOSS_CASES:
        cs = [cases[k] for k in names]
        A, st = cs[0]["A"], cs[0]["cfg"]["stride"]
        S, Hh, W = cs[0]["im_size"]
        lg, pr = loss_inputs(lseed, len(cs), A, S // st, Hh // st, W // st)
        tl, tp = torch.tensor(lg, requires_grad=True), torch.tensor(pr, requires_grad=True)
        cat = lambda k: torch.from_numpy(np.concatenate([np.ascontiguousarray(c["blobs"][k]) for c in cs], 0))  # noqa: E731
        lc, lb = RH.single_scale_rpn_losses(tl, tp, cat("rpn_labels_int32_wide"), cat("rpn_bbox_targets_wide"),
                                            cat("rpn_bbox_inside_weights_wide"), cat("rpn_bbox_outside_weights_wide"))
        gl, = torch.autograd.grad(lc, tl, retain_graph=True)
        gp, = torch.autograd.grad(lb, tp)
        out[lname + "_seed"] = np.array(lseed, np.int64)
        out[lname + "_losses"] = np.array([lc.item(), lb.item()], np.float32)
        out[lname + "_grad_logits"], out[lname + "_grad_pred"] = gl.numpy(), gp.numpy()
        print(lname, lc.item(), lb.item())
    torch.set_num_threads(threads)
    return out


def write(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    path = os.path.join(HERE, "rpn_train.npz")
    write(path, build_arrays())
    print("wrote", path, os.path.getsize(path), "bytes")
