"""Golden vectors for the training-sample path: runs the REFERENCE's own `utils.blob.prep_im_for_blob(..., 'train')` (and through it
`crop_data_3d`) and `_load_ann_objs` + `_add_gt_annotations` of both dataset classes on the CPU through oracle/ref_harness.py, and writes
tests/golden/train_sample.npz.

`utils.blob.npr` is replaced by an object whose `choice` implements the sampling contract of DESIGN ("Training samples"): the start of
axis a is `(key(stream(seed), a) * len(range)) >> 32`.  The dataset methods are called on an object that carries only the attributes
they read; annotation files are written to a temporary directory and `io.imread` of the nuclei module reads the mask from there.

Each case stores data only: inputs, seed, chosen origin, kept boxes and indices (`seg_volumes` carries the box index through the
reference's filter).  The generator asserts what each case exists for, and that tests/train_sample_reference.py gives the same result.

Run in the build container only:  python tests/golden/gen_train_sample.py"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"),
          os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import train_sample_reference as R  # noqa: E402
from rpn_train_reference import key, stream  # noqa: E402
from gen_rpn_train import write  # noqa: E402

SOMA = "configs/soma_starting/e2e_mask_rcnn_soma_dsn_body.yaml"
NUC = "configs/cell_tracking_baseline/e2e_mask_rcnn_N3DH_SIM_dsn_body.yaml"
IN_SIZE = (8, 16, 12)


class FakeNpr:
    """npr.choice(range(0, start_max + 1)) of blob.py:115-120: called for x, y, z in turn, but only where start_max != 0"""

    def __init__(self, seed, smax):
        self.stream, self.axes, self.smax, self.draws = stream(seed), [a for a in range(3) if smax[a] != 0], smax, 0

    def choice(self, r):
        a = self.axes.pop(0)
        assert len(r) == self.smax[a] + 1 and r[0] == 0
        self.draws += 1
        return r[(int(key(self.stream, a)) * len(r)) >> 32]


def int_boxes(rng, K, dims, lo=1, hi=9):
    D, H, W = dims
    c = np.stack([rng.randint(0, W, K), rng.randint(0, H, K), rng.randint(0, D, K)], 1)
    r = rng.randint(lo, hi, (K, 3))
    b = np.concatenate([np.maximum(c - r, 0), np.minimum(c + r, np.array([W, H, D]) - 1)], 1).astype(np.float32)
    return b[(b[:, 3] > b[:, 0]) & (b[:, 4] > b[:, 1]) & (b[:, 5] > b[:, 2])]


def crop_cases():
    """name, dims (D,H,W), boxes, seed, need_crop"""
    rng = np.random.RandomState(7)
    cases = [
        # every axis draws: the lowest box corner is at (5, 7, 3) and the volume leaves room on every axis
        ("draw3", (20, 40, 30), np.array([[5, 7, 3, 12, 15, 9], [14, 20, 8, 25, 33, 15], [8, 30, 12, 20, 38, 18]], np.float32), 11, True),
        # start_max == 0 on x (a box touches x = 0) and on z (depth == IN_SIZE[0])
        ("axis0", (8, 40, 30), np.array([[0, 9, 1, 6, 15, 5], [15, 22, 2, 27, 34, 7]], np.float32), 12, True),
        # a dropped box: the far box cannot share a crop with the two near ones
        ("drop", (8, 16, 40), np.array([[0, 2, 1, 7, 9, 6], [3, 5, 0, 10, 14, 7], [34, 3, 2, 39, 10, 6]], np.float32), 13, True),
        # a tie: the crops at x = 0 and x = 12 hold one 6 x 6 x 6 box each, the one between them none
        ("tie", (8, 16, 24), np.array([[0, 4, 1, 5, 9, 6], [18, 4, 1, 23, 9, 6]], np.float32), 14, True),
        # the volume is exactly IN_SIZE: one candidate
        ("full", IN_SIZE, np.array([[1, 2, 1, 6, 9, 5], [4, 6, 2, 11, 15, 7]], np.float32), 15, True),
        # the nuclei yaml: no crop, the boxes untouched - degenerate ones included
        ("nocrop", IN_SIZE, np.array([[1, 2, 1, 6, 9, 5], [4, 6, 2, 4, 15, 7]], np.float32), 16, False),
    ]
    for i in range(12):
        dims = (int(rng.randint(8, 31)), int(rng.randint(16, 51)), int(rng.randint(12, 41)))
        b = int_boxes(rng, int(rng.randint(2, 12)), dims)
        if len(b):
            cases.append(("rand%d" % i, dims, b, 100 + i, True))
    return cases


def run_crop(H, name, dims, boxes, seed, need_crop):
    import utils.blob as B
    cfg = H.load_cfg(SOMA if need_crop else NUC, ("TRAIN.IN_SIZE", IN_SIZE, "TRAIN.NEED_CROP", need_crop))
    assert B.cfg is cfg
    K = len(boxes)
    smax = R.start_max(boxes, dims, IN_SIZE)
    fake = FakeNpr(seed, smax)
    B.npr = fake
    rng = np.random.RandomState(seed)
    im = rng.randint(1, 4000, dims).astype(np.uint16)
    classes = np.ones(K, np.int32)
    crowd = (np.arange(K) % 3 == 1)
    entry = dict(boxes=boxes.copy(), segms=np.zeros((K, 4), np.float32), gt_classes=classes.copy(), is_crowd=crowd.copy(),
                 seg_volumes=np.arange(K, dtype=np.float32))
    ims, scales = B.prep_im_for_blob(im, entry, "train")
    assert scales == [1.0] and ims[0].shape == tuple(IN_SIZE) and ims[0].dtype == np.float32
    keep = entry["seg_volumes"].astype(np.int32)
    assert np.array_equal(entry["gt_classes"], classes[keep]) and np.array_equal(entry["is_crowd"], crowd[keep])
    got = R.sample(boxes, dims, IN_SIZE, seed, need_crop=need_crop)
    n = int(got["info"][3])
    if need_crop:
        # the reference's origin: the crop it returns is that window of the normalised volume
        f = im.astype(np.float32)
        m = f > 0
        full = (f - np.mean(f[m])) / np.std(f[m])
        assert np.array_equal(R.crop(full, got["origin"], IN_SIZE), ims[0]), name
        assert fake.draws == sum(1 for v in smax if v != 0) and not fake.axes
    assert n == len(keep) and np.array_equal(got["keep"][:n], keep) and np.array_equal(got["boxes"][:n], entry["boxes"]), name
    return dict(dims=np.array(dims, np.int64), boxes=boxes, seed=np.array(seed, np.int64), need_crop=np.array(int(need_crop), np.int64),
                origin=np.array(got["origin"], np.int64), kept_boxes=entry["boxes"].astype(np.float32), keep=keep,
                classes=classes, crowd=crowd, kept_classes=entry["gt_classes"].astype(np.int32), kept_crowd=entry["is_crowd"].astype(bool),
                start_max=np.array(smax, np.int64), score=np.array(got["score"], np.float64)), got


SOMA_TXT = ["x y z r\n", "10 12 6 3\n", "30 40 20 4\n", "2 1 1 5\n", "22 30 14 0\n", "23 31 15 2\n", "12 20 8 6"]
NUC_MIXED = ["id x y z w h s marker\n", "1 5.0 6.0 2.0 8 9 5 1\n", "2 0 10 3 6 8 4 2\n", "3 12 0 1 30 7 6 3\n", "4 14 12 8 6 6 4 9\n",
             "5 14 20.7 9 7 8 5 5\n", "6 0 2 10 5 5 4 6"]
NUC_LAST = ["id x y z w h s marker\n", "1 0 3 2 6 8 5 1\n", "2 10 0 4 9 7 4 2\n", "3 0 20 8 8 9 5 3"]
ANN_IM_SIZE = (16, 32, 24)


def nuclei_mask(lines):
    """every marker but 9 fills its box: marker 9 has no voxel and its line is dropped"""
    S, H, W = ANN_IM_SIZE
    mask = np.zeros(ANN_IM_SIZE, np.uint8)
    for a in lines[1:]:
        p = a.rstrip().split(" ")
        x, y, z, w, h, s, m = [int(float(v)) for v in p[1:8]]
        if m != 9:
            mask[z + 1:z + s, y:y + h, x:x + w] = m
    return mask


def entry_of(num_classes=2):
    import scipy.sparse
    return dict(boxes=np.empty((0, 6), np.float32), gt_classes=np.empty(0, np.int32), seg_volumes=np.empty(0, np.float32),
                gt_overlaps=scipy.sparse.csr_matrix(np.empty((0, num_classes), np.float32)), is_crowd=np.empty(0, bool),
                box_to_gt_ind_map=np.empty(0, np.int32))


def run_readers(H, out):
    tmp = tempfile.mkdtemp()
    # ---- soma
    H.load_cfg(SOMA, ("TRAIN.IM_SIZE", ANN_IM_SIZE))
    import datasets.soma_dataset as SD
    import core.config as CC
    ratio = CC.cfg.TRAIN.RADIUS_EXP_RATIO
    with open(os.path.join(tmp, "s0.txt"), "w") as f:
        f.writelines(SOMA_TXT)

    class Soma:
        _load_ann_objs = SD.SomaDataset._load_ann_objs
        _add_gt_annotations = SD.SomaDataset._add_gt_annotations
        label_directory, category_to_id_map, num_classes = tmp, {"soma": 1}, 2
    e = entry_of()
    e["file_name"], e["segms"] = "s0", np.empty((0, 4), np.float32)
    Soma()._add_gt_annotations(e)
    b, c, cr, sg, v = R.read_soma(SOMA_TXT, ANN_IM_SIZE, ratio)
    assert np.array_equal(b, e["boxes"]) and np.array_equal(c, e["gt_classes"]) and np.array_equal(cr, e["is_crowd"])
    assert np.array_equal(sg, e["segms"]) and np.array_equal(v, e["seg_volumes"])
    assert len(b) == len(SOMA_TXT) - 2, "the radius-0 soma is dropped"
    assert (b[:, :3] == 0).any() and (b[:, 3] == ANN_IM_SIZE[2] - 1).any(), "boxes clamped at both ends"
    assert int(SOMA_TXT[2].split()[0]) > ANN_IM_SIZE[2] - 1, "a centre outside IM_SIZE"
    out.update(soma_text=np.frombuffer("".join(SOMA_TXT).encode(), np.uint8), soma_im_size=np.array(ANN_IM_SIZE, np.int64),
               soma_ratio=np.array(ratio, np.float64), soma_boxes=e["boxes"], soma_classes=e["gt_classes"].astype(np.int32),
               soma_crowd=e["is_crowd"].astype(bool), soma_segms=e["segms"], soma_volumes=e["seg_volumes"])
    # ---- nuclei
    H.load_cfg(NUC, ("TRAIN.IM_SIZE", ANN_IM_SIZE))
    import datasets.nuclei_dataset as ND
    ND.io = types.SimpleNamespace(imread=lambda path: np.load(path[:-4] + ".npy"))
    ND.binary_mask_to_rle = lambda m: None
    os.makedirs(os.path.join(tmp, "bbox"))
    os.makedirs(os.path.join(tmp, "mask"))

    class Nuclei:
        _load_ann_objs = ND.NucleiDataset._load_ann_objs
        _add_gt_annotations = ND.NucleiDataset._add_gt_annotations
        label_directory, category_to_id_map, num_classes = tmp, {"nuclei": 1}, 2
    for name, lines in (("nuc_mixed", NUC_MIXED), ("nuc_last", NUC_LAST)):
        mask = nuclei_mask(lines)
        with open(os.path.join(tmp, "bbox", name + ".txt"), "w") as f:
            f.writelines(lines)
        np.save(os.path.join(tmp, "mask", name + ".npy"), mask)
        e = entry_of()
        e["file_name"], e["segms"] = name, []
        Nuclei()._add_gt_annotations(e)
        b, c, cr, v = R.read_nuclei(lines, mask, ANN_IM_SIZE)
        assert np.array_equal(b, e["boxes"]) and np.array_equal(c, e["gt_classes"]) and np.array_equal(cr, e["is_crowd"])
        assert np.array_equal(v, e["seg_volumes"])
        out.update({name + "_text": np.frombuffer("".join(lines).encode(), np.uint8), name + "_mask": mask,
                    name + "_im_size": np.array(ANN_IM_SIZE, np.int64), name + "_boxes": e["boxes"],
                    name + "_classes": e["gt_classes"].astype(np.int32), name + "_crowd": e["is_crowd"].astype(bool),
                    name + "_volumes": e["seg_volumes"]})
    mixed, last = out["nuc_mixed_crowd"], out["nuc_last_crowd"]
    assert len(mixed) == len(NUC_MIXED) - 2, "the line whose marker has no voxel is dropped"
    assert list(mixed) == [False, True, True, False, True], "crowd by x, crowd by y, and a border box on the last line after a kept nucleus"
    assert list(last) == [True, True, False], "the last line: at the border like the others, but nothing before it was kept"


def build_arrays():
    import ref_harness as H
    H.install()
    out, got = {}, {}
    names = []
    for name, dims, boxes, seed, need_crop in crop_cases():
        arrays, got[name] = run_crop(H, name, dims, boxes, seed, need_crop)
        for k, v in arrays.items():
            out["%s_%s" % (name, k)] = v
        names.append(name)
        print(name, dims, "start_max", tuple(arrays["start_max"]), "origin", tuple(arrays["origin"]), "kept", len(arrays["keep"]), "of", len(boxes))
    out["names"] = np.frombuffer(",".join(names).encode(), np.uint8)
    out["in_size"] = np.array(IN_SIZE, np.int64)

    # ---- the properties the cases exist for
    def scores(name):
        c = [c for c in crop_cases() if c[0] == name][0]
        return R.search(c[2], R.candidates(R.draw_starts(c[3], R.start_max(c[2], c[1], IN_SIZE)), c[1], IN_SIZE), IN_SIZE)
    assert all(v > 0 for v in out["draw3_start_max"]), "a draw on each axis"
    sm = out["axis0_start_max"]
    assert sm[0] == 0 and sm[2] == 0 and sm[1] > 0, "axes with start_max == 0 beside one that draws"
    assert len(out["drop_keep"]) < len(out["drop_boxes"]), "a dropped box"
    o, best, status, sc = scores("tie")
    assert sorted(sc)[-1] == sorted(sc)[-2] == best and sc.index(best) == 0 and tuple(out["tie_origin"]) == (0, 0, 0), "a tie; the first wins"
    assert tuple(out["full_dims"]) == IN_SIZE and len(scores("full")[3]) == 1, "volume == IN_SIZE"
    assert np.array_equal(out["nocrop_kept_boxes"], out["nocrop_boxes"]) and (out["nocrop_boxes"][:, 0] == out["nocrop_boxes"][:, 3]).any()
    assert any(len(out["rand%d_keep" % i]) < len(out["rand%d_boxes" % i]) for i in range(12) if "rand%d_keep" % i in out)
    for n in names:      # the fp32 / fp64 note: integer coordinates, sums below 2^24
        assert np.array_equal(out[n + "_boxes"], np.round(out[n + "_boxes"])) and out[n + "_score"] < 2 ** 24
    run_readers(H, out)
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "train_sample.npz")
    write(path, build_arrays())
    print("wrote", path, os.path.getsize(path), "bytes")
