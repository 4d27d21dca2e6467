#!/usr/bin/env python3
"""Generates tests/golden/eval_baselines.npz by RUNNING THE REFERENCE'S OWN SCRIPT tools/evaluation/
eval_instance_segmentation_soma_ngps.py (CPU) for both of its flags, 'DSN' and 'NGPS', at IoU thresholds 0.3, 0.5 and 0.7.

Run in the build container only (needs the reference tree; default /root/reference, or $M3D_REFERENCE):
    python tests/golden/gen_eval_baselines.py
The module is imported under stubs: numba.jit is the identity (mask_iou_fast runs as plain Python), skimage.io.imread reads through
m3d.io.read_tiff_stack, np.float / np.bool are aliased, and skimage.measure.label is stubbed, because skimage is not installed where
this runs.  THE LABELLING ITSELF IS THEREFORE PINNED BY SCIPY, NOT BY A RUN OF SKIMAGE: the stub is an independent restatement of
skimage.measure.label's default semantics - scipy.ndimage.label with the full 3x3x3 structure once per distinct non-zero value, the
components then renumbered by their first raster index.  Everything downstream of it (the size filter, the sphere painting, the IoU,
the matching, precision / recall / AP) is the reference's own code.  mask_iou_fast is a P x G x V Python loop that does not depend
on the threshold; its results are memoised per input so that the six calls per flag pay for it once.
calc_instance_segmentation_voc_prec_rec and eval_instance_segmentation_soma are both called; the ids that survive the script's size
filter and its per-image APs are read from the running function's locals with a line tracer (the script returns neither).

Inputs: three 24 x 64 x 64 images from m3d.synth.synth_label_pair(shape, 6, seed), seeds 100..102.
  DSN   (pred > 0) * 255 as uint8 plus 40 seeded single-voxel specks per image: the specks fall below the script's 300-voxel filter,
        and the filter's skip-after-remove quirk lets about half of them through.
  NGPS  one SWC line per GT instance (centroid jittered, equivalent radius +- 1.5), plus a sphere with r >= 6 hugging the low corner
        (the clamp at index 1; its x centre is negative: int(float(.)) truncates toward zero), one with r < 6 (the id counter
        skips) and a sphere overlapping the first instance's (the later id overwrites).
Only arrays are stored (inputs, SWC text as bytes, sphere tables, surviving ids, the script's prec / rec / ap); the zip is written
with fixed timestamps, so a re-run reproduces the file bit for bit."""
import contextlib
import hashlib
import inspect
import io
import os
import sys
import tempfile
import types
import zipfile

import numpy as np
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
from m3d.io import read_tiff_stack, write_tiff_stack  # noqa: E402
from m3d.synth import synth_label_pair  # noqa: E402

REF = os.environ.get("M3D_REFERENCE", "/root/reference")
EVAL = os.path.join(REF, "tools", "evaluation")
SHAPE = (24, 64, 64)
SEEDS = (100, 101, 102)
THRESHOLDS = (0.3, 0.5, 0.7)
SPECKS = 40


def label_stub(x):
    """skimage.measure.label(x) with default arguments, restated on SciPy: components of equal non-zero value, full connectivity,
    numbered by the raster index of their first voxel."""
    x = np.asarray(x)
    full = np.ones((3,) * x.ndim, bool)
    comps = []
    for val in np.unique(x):
        if val == 0:
            continue
        lab, n = ndimage.label(x == val, structure=full)
        ids, first = np.unique(lab.ravel(), return_index=True)
        comps += [(int(f), lab, int(i)) for i, f in zip(ids, first) if i != 0]
    out = np.zeros(x.shape, np.int64)
    for k, (_, lab, i) in enumerate(sorted(comps, key=lambda c: c[0])):
        out[lab == i] = k + 1
    return out


def stubs():
    nb = types.ModuleType("numba")
    nb.jit = lambda *a, **k: (lambda f: f)
    sk = types.ModuleType("skimage")
    skio = types.ModuleType("skimage.io")
    skio.imread = read_tiff_stack
    skm = types.ModuleType("skimage.measure")
    skm.label = label_stub
    sk.io, sk.measure = skio, skm
    sys.modules.update({"numba": nb, "skimage": sk, "skimage.io": skio, "skimage.measure": skm})
    if not hasattr(np, "float"):
        np.float = float
    if not hasattr(np, "bool"):
        np.bool = bool


def memoised(fn):
    cache = {}

    def call(a, b):
        key = hashlib.sha256(a.tobytes() + b"|" + b.tobytes() + repr((a.shape, b.shape)).encode()).hexdigest()
        if key not in cache:
            cache[key] = fn(a, b)
        return cache[key].copy()
    return call


def make_images():
    imgs = []
    for seed in SEEDS:
        gt, pred, _ = synth_label_pair(SHAPE, 6, seed)
        rng = np.random.RandomState(1000 + seed)
        dsn = ((pred > 0) * 255).astype(np.uint8)
        flat = dsn.reshape(-1)
        flat[rng.choice(flat.size, SPECKS, replace=False)] = 255
        lines, n = [], 0
        for i in np.unique(gt)[1:]:
            z, y, x = np.nonzero(gt == i)
            r = (3.0 * z.size / (4.0 * np.pi)) ** (1.0 / 3.0) + rng.uniform(-1.5, 1.5)
            c = np.array([x.mean(), y.mean(), z.mean()]) + rng.uniform(-1.5, 1.5, 3)
            n += 1
            lines.append("%d 1 %.3f %.3f %.3f %.3f -1" % (n, c[0], c[1], c[2], r))
            if n == 1:
                first = (c, r)
        extra = [(-0.7, 2.2, 1.9, 7.6),                                                 # hugs the low corner: the clamp at 1 shows
                 (40.5, 40.5, 12.5, 5.9),                                               # r < 6: paints nothing, the counter advances
                 (first[0][0] + 4.0, first[0][1] - 3.0, first[0][2] + 1.0, max(first[1], 6.5))]   # overlaps instance 1: overwrites
        for e in extra:
            n += 1
            lines.append("%d 1 %.3f %.3f %.3f %.3f -1" % ((n,) + e))
        imgs.append((gt.astype(np.uint16), dsn, "\n".join(lines) + "\n"))
    return imgs


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


class Probe:
    """Reads pred_mask_ids (after the filter) and ap_single from the frame of calc_instance_segmentation_voc_prec_rec while it runs."""

    def __init__(self, fn):
        src, first = inspect.getsourcelines(fn)
        self.code = fn.__code__
        self.ids_line = first + next(k for k, s in enumerate(src) if "gt_mask_ids = np.unique(gt_mask)" in s)
        self.ap_line = first + next(k for k, s in enumerate(src) if "fid.write('{}: {:.4f}" in s) - 1
        self.ids, self.aps = [], []

    def local(self, frame, event, arg):
        if event == "line" and frame.f_lineno == self.ids_line:
            self.ids.append(np.array(frame.f_locals["pred_mask_ids"], dtype=np.int64))
        elif event == "line" and frame.f_lineno == self.ap_line:
            self.aps.append(float(frame.f_locals["ap_single"]))
        return self.local

    def __call__(self, frame, event, arg):
        return self.local if frame.f_code is self.code else None


def main():
    stubs()
    sys.path.insert(0, EVAL)
    import mask_iou as M
    M.mask_iou_fast = memoised(M.mask_iou_fast)
    import eval_instance_segmentation_soma_ngps as S
    imgs = make_images()
    names = ["img%d" % k for k in range(len(imgs))]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gdir = os.path.join(tmp, "gt")
        pdir = {"DSN": os.path.join(tmp, "dsn"), "NGPS": os.path.join(tmp, "ngps")}
        for d in pdir.values():
            os.makedirs(d)
        for name, (gt, dsn, swc) in zip(names, imgs):
            os.makedirs(os.path.join(gdir, name))
            write_tiff_stack(os.path.join(gdir, name, name + ".tif"), gt)
            write_tiff_stack(os.path.join(pdir["DSN"], name + ".tif"), dsn)
            with open(os.path.join(pdir["NGPS"], name + ".swc"), "w") as f:
                f.write(swc)
        for flag in ("DSN", "NGPS"):
            for t in THRESHOLDS:
                tag = "%s_%s" % (flag.lower(), ("%g" % t).replace(".", ""))
                probe = Probe(S.calc_instance_segmentation_voc_prec_rec)
                with contextlib.redirect_stdout(io.StringIO()):
                    sys.settrace(probe)
                    try:
                        prec, rec = S.calc_instance_segmentation_voc_prec_rec(flag, pdir[flag], gdir, names, t)
                    finally:
                        sys.settrace(None)
                    res = S.eval_instance_segmentation_soma(flag, pdir[flag], gdir, names, t)
                assert len(probe.ids) == len(imgs) == len(probe.aps) and all(len(i) for i in probe.ids)
                out[tag + "_prec"], out[tag + "_rec"] = prec, rec
                out[tag + "_ap"] = np.float64(res["ap"])
                assert np.float64(S.voc_ap(rec, prec)[2]).tobytes() == np.float64(res["ap"]).tobytes()
                out[tag + "_per_image_ap"] = np.array(probe.aps, np.float64)
                for k, ids in enumerate(probe.ids):
                    key = "%s_ids_%d" % (flag.lower(), k)
                    assert key not in out or np.array_equal(out[key], ids)              # the filter does not depend on the threshold
                    out[key] = ids
    for k, (gt, dsn, swc) in enumerate(imgs):
        out["gt_%d" % k], out["dsn_%d" % k] = gt, dsn
        out["swc_%d" % k] = np.frombuffer(swc.encode("ascii"), np.uint8)
        out["spheres_%d" % k] = np.array([[int(float(v)) for v in ln.split(" ")[2:6]] for ln in swc.rstrip().split("\n")], np.int64)
    p = os.path.join(HERE, "eval_baselines.npz")
    write_npz(p, out)
    print("wrote eval_baselines.npz (%.1f KB); rows per image DSN %s NGPS %s; AP DSN %s NGPS %s" % (
        os.path.getsize(p) / 1024, [len(out["dsn_ids_%d" % k]) for k in range(len(imgs))],
        [len(out["ngps_ids_%d" % k]) for k in range(len(imgs))],
        [float(out["dsn_%s_ap" % ("%g" % t).replace(".", "")]) for t in THRESHOLDS],
        [float(out["ngps_%s_ap" % ("%g" % t).replace(".", "")]) for t in THRESHOLDS]))


if __name__ == "__main__":
    main()
