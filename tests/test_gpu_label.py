"""GPU: whole-volume labelling and sphere painting (csrc/label3d.hip), the baseline scoring built on them (m3d.evaluate_baselines,
tools/evaluate.py soma-dsn | soma-ngps) and tools/label_volume.py - against scipy.ndimage.label, the NumPy / SciPy restatement of
the reference's script (tests/baseline_reference.py) and the script's own results (tests/golden/eval_baselines.npz).  Everything is
compared exactly: labels and counts are integers, and the scoring arithmetic is the reference's NumPy operations."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from scipy import ndimage

import baseline_reference as B
import m3d
from m3d import evaluate_baselines as EB
from m3d import ops
from m3d.io import read_tiff_stack, write_tiff_stack
from m3d.synth import synth_label_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "eval_baselines.npz")
TAGS = {0.3: "03", 0.5: "05", 0.7: "07"}
CONNS = (6, 18, 26)
N = 3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def check_binary(mask, conns=CONNS):
    """label_components == scipy.ndimage.label exactly, K and the counts included"""
    mask = np.ascontiguousarray(mask)
    for c in conns:
        want, k = ndimage.label(mask, structure=ndimage.generate_binary_structure(3, B.RANK[c]))
        labels, K, counts = m3d.label_components(mask, c, return_counts=True)
        got = labels.cpu().numpy()
        assert labels.dtype == torch.int32 and tuple(labels.shape) == mask.shape
        assert K == k, (mask.shape, c, K, k)
        assert np.array_equal(got, want), (mask.shape, c)
        assert K == int(got.max(initial=0))
        assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), np.bincount(got.ravel(), minlength=K + 1))


def serpentine(shape):
    """a one-voxel-wide path that snakes through the whole volume: whole x rows on every second y of every second plane, each joined
    to the next by one voxel at the end the walk has reached (the longest union-find chains)"""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    x_end = 0                                            # the walk enters each row here and leaves at the other end
    ys = list(range(0, H, 2))
    for i, z in enumerate(range(0, D, 2)):
        order = ys if i % 2 == 0 else ys[::-1]
        for j, y in enumerate(order):
            m[z, y, :] = 1
            x_end = W - 1 - x_end
            if j + 1 < len(order):
                m[z, (y + order[j + 1]) // 2, x_end] = 1
        if z + 2 < D:
            m[z + 1, order[-1], x_end] = 1
    return m


@pytest.mark.parametrize("density", [0.05, 0.12, 0.31, 0.6])
@pytest.mark.parametrize("shape", [(1, 1, 200), (200, 1, 1), (5, 7, 9), (3, 5, 63), (3, 5, 65), (2, 17, 255), (2, 9, 257), (4, 16, 64),
                                   (5, 17, 65), (3, 31, 33), (9, 33, 130), (1, 1, 1023), (1, 1, 1025), (1, 16, 64), (3, 341, 1), (2, 8, 2049)])
# the kernel's edges: waves of 64 voxels, workgroups of 256, scan blocks of 1 024 voxels - x rows and volumes one below and one above each
def test_random_masks(shape, density):
    rng = np.random.RandomState(int(density * 100) + shape[2])
    check_binary((rng.uniform(size=shape) < density).astype(np.uint8))


@pytest.mark.parametrize("shape", [(96, 256, 256), (59, 350, 350)])
@pytest.mark.parametrize("density", [0.05, 0.12, 0.31, 0.6])
def test_random_masks_full_size(shape, density):
    rng = np.random.RandomState(7)
    check_binary((rng.uniform(size=shape) < density).astype(np.uint8))


@pytest.mark.parametrize("shape", [(96, 256, 256), (59, 350, 350)])
def test_blobs_full_size(shape):
    _, pred, _ = synth_label_pair(shape, 40, 3)
    check_binary(((pred > 0) * 255).astype(np.uint8), conns=(26,))


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 9), (4, 16, 64), (3, 33, 129), (7, 40, 300)])
def test_special_masks(shape):
    check_binary(np.zeros(shape, np.uint8))
    check_binary(np.ones(shape, np.uint8))
    one = np.zeros(shape, np.uint8)
    one[shape[0] // 2, shape[1] // 2, shape[2] // 2] = 200
    check_binary(one)
    zz, yy, xx = np.indices(shape)
    board = ((zz + yy + xx) % 2 == 0).astype(np.uint8)
    check_binary(board)
    V = int(np.prod(shape))
    assert m3d.label_components(board, 6)[1] == (V + 1) // 2
    assert m3d.label_components(board, 26)[1] == 1
    snake = serpentine(shape)
    check_binary(snake)
    assert m3d.label_components(snake, 6)[1] == 1


def test_serpentine_full_size():
    snake = serpentine((96, 256, 256))
    check_binary(snake, conns=(6, 26))


def test_bool_and_cuda_inputs():
    rng = np.random.RandomState(5)
    m = rng.uniform(size=(6, 20, 70)) < 0.3
    want = ndimage.label(m, structure=np.ones((3, 3, 3), bool))[0]
    for x in (m, m.astype(np.uint8), torch.from_numpy(m).cuda(), torch.from_numpy(m.astype(np.uint8)).cuda(),
              torch.from_numpy(m.astype(np.int32) * 70000).cuda(), (m * 300).astype(np.uint16)):
        assert np.array_equal(m3d.label_components(x)[0].cpu().numpy(), want)
    nc = torch.from_numpy(m.astype(np.uint8)).cuda().permute(0, 2, 1)             # non-contiguous input
    assert np.array_equal(m3d.label_components(nc)[0].cpu().numpy(), ndimage.label(m.transpose(0, 2, 1), structure=np.ones((3, 3, 3), bool))[0])


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.int32])
@pytest.mark.parametrize("conn", CONNS)
def test_multi_valued(dtype, conn):
    rng = np.random.RandomState(11)
    top = {np.uint8: 255, np.uint16: 65535, np.int32: 2 ** 31 - 1}[dtype]
    vals = np.array([0, 0, 1, 2, top], dtype=np.int64)
    x = vals[rng.randint(0, len(vals), (6, 21, 67))].astype(dtype)
    want, k = B.label(x, conn)
    labels, K = m3d.label_components(x, conn)
    assert K == k and np.array_equal(labels.cpu().numpy(), want)
    # coarser regions: a label volume relabelled
    gt, pred, _ = synth_label_pair((12, 40, 70), 9, 2)
    x = (pred.astype(np.int64) % 3 + (pred > 0)).astype(dtype)
    want, k = B.label(x, conn)
    labels, K, counts = m3d.label_components(x, conn, return_counts=True)
    assert K == k and np.array_equal(labels.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(want.ravel(), minlength=k + 1))


def test_value_semantics():
    x = np.zeros((3, 4, 6), np.uint8)
    x[0, 0, 0:2] = 5
    x[0, 0, 2:4] = 9                 # touches the 5s: a different value, so a different component
    x[1, 1, 4] = 9                   # touches x[0, 0, 3] only diagonally
    l26, k26 = m3d.label_components(x, 26)
    l18, k18 = m3d.label_components(x, 18)
    l6, k6 = m3d.label_components(x, 6)
    l26, l18, l6 = l26.cpu().numpy(), l18.cpu().numpy(), l6.cpu().numpy()
    assert k26 == 2 and l26[0, 0, 0] == l26[0, 0, 1] == 1 and l26[0, 0, 2] == l26[0, 0, 3] == l26[1, 1, 4] == 2
    assert k18 == 3 and l18[1, 1, 4] == 3          # a corner neighbour (three coordinates differ) joins at 26 only
    assert k6 == 3 and l6[1, 1, 4] == 3
    y = np.zeros((2, 3, 3), np.uint16)
    y[0, 0, 0] = y[0, 1, 1] = 7      # an edge neighbour (two coordinates differ): joins at 18 and 26, not at 6
    assert [m3d.label_components(y, c)[1] for c in CONNS] == [2, 1, 1]


def test_bit_identical_runs():
    rng = np.random.RandomState(3)
    m = (rng.uniform(size=(40, 128, 160)) < 0.2).astype(np.uint8)
    d = torch.from_numpy(m).cuda()
    a, ka, ca = m3d.label_components(d, 26, return_counts=True)
    b, kb, cb = m3d.label_components(d, 26, return_counts=True)
    assert ka == kb and torch.equal(a, b) and torch.equal(ca, cb)


def test_label_counts_solid_and_out_of_range():
    lab = torch.zeros((8, 64, 100), dtype=torch.int32, device="cuda")
    lab[2:6, 10:50, 3:97] = 2
    lab[0, 0, 0] = 9                                                              # above num_labels: not counted, not indexed
    c = m3d.label_counts(lab, 3).cpu().numpy()
    assert c.tolist() == [8 * 64 * 100 - 4 * 40 * 94 - 1, 0, 4 * 40 * 94, 0]


def test_rejects_bad_input():
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((2, 2, 2, 2), np.uint8), np.zeros((2, 3, 4), np.float32), np.zeros((2, 3, 4), np.int64),
                torch.zeros((2, 3, 4), dtype=torch.float32, device="cuda"), torch.zeros((3, 4), dtype=torch.uint8, device="cuda")):
        with pytest.raises(ValueError):
            m3d.label_components(bad)


def test_argument_checks():
    x = torch.zeros((2, 3, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(m3d.M3DError, match=r"\(-4\)"):                            # M3D_EUNSUPPORTED: >= 2^31 voxels, by shape alone
        ops._label_components_raw(x, 1, 2048, 1024, 1024, 26)
    with pytest.raises(m3d.M3DError, match=r"\(-4\)"):
        ops._label_components_raw(x, 1, 2, 2 ** 15, 2 ** 15, 26)                 # exactly 2^31
    for nbytes, dims, conn in ((1, (2, 3, 4), 8), (1, (2, 3, 4), 0), (3, (2, 3, 4), 26), (8, (2, 3, 4), 26), (1, (0, 3, 4), 26),
                               (1, (2, 0, 4), 26), (1, (2, 3, 0), 26), (1, (2, 3, -1), 26)):
        with pytest.raises(m3d.M3DError, match=r"\(-1\)"):                        # M3D_EINVAL
            ops._label_components_raw(x, nbytes, dims[0], dims[1], dims[2], conn)
    with pytest.raises(m3d.M3DError, match=r"\(-1\)"):
        m3d.paint_spheres(np.zeros((65536, 4), np.int64), (4, 8, 8))
    assert int(m3d.paint_spheres(np.zeros((0, 4), np.int64), (4, 8, 8)).to(torch.int32).abs().sum()) == 0


# ------------------------------------------------------------------ sphere painting
def check_spheres(sp, shape):
    got = m3d.paint_spheres(sp, shape)
    assert got.dtype == torch.uint16 and tuple(got.shape) == tuple(shape)
    assert np.array_equal(got.cpu().numpy(), B.paint_spheres(sp, shape))


@pytest.mark.parametrize("k", range(N))
def test_paint_spheres_golden(g, k):
    check_spheres(g["spheres_%d" % k], g["gt_%d" % k].shape)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_paint_spheres_random(seed):
    rng = np.random.RandomState(seed)
    shape = (20, 50, 70)
    n = 60
    sp = np.stack([rng.randint(-15, 85, n), rng.randint(-15, 65, n), rng.randint(-15, 35, n), rng.randint(0, 14, n)], 1)
    sp[0] = (200, 200, 200, 9)                       # wholly outside
    sp[1] = (-30, 10, 10, 8)
    sp[2] = (35, 25, 10, 60)                         # covers the whole volume (an early id: later spheres overwrite it)
    sp[3] = (0, 0, 0, 6)
    check_spheres(sp, shape)
    check_spheres(sp[::-1].copy(), shape)


# ------------------------------------------------------------------ the two baseline evaluations
def baseline_inputs(g, flag):
    gts = [g["gt_%d" % k] for k in range(N)]
    if flag == "dsn":
        preds = [m3d.label_components(g["dsn_%d" % k])[0] for k in range(N)]
    else:
        preds = [m3d.paint_spheres(g["spheres_%d" % k], gts[k].shape) for k in range(N)]
    return preds, gts


@pytest.mark.parametrize("flag", ["dsn", "ngps"])
@pytest.mark.parametrize("t", sorted(TAGS))
def test_baseline_core_matches_reference(g, flag, t):
    preds, gts = baseline_inputs(g, flag)
    prec, rec, per, ids = EB.baseline_prec_rec(preds, gts, t)
    tag = "%s_%s" % (flag, TAGS[t])
    assert np.array_equal(bits(prec), bits(g[tag + "_prec"]))
    assert np.array_equal(bits(rec), bits(g[tag + "_rec"]))
    assert bits(EB.voc_ap(rec, prec)[2]) == bits(g[tag + "_ap"])
    assert np.array_equal(bits(per), bits(g[tag + "_per_image_ap"]))
    assert [i.tolist() for i in ids] == [g["%s_ids_%d" % (flag, k)].tolist() for k in range(N)]


def baseline_tree(g, tmp):
    gdir, ddir, sdir = os.path.join(tmp, "gt"), os.path.join(tmp, "dsn"), os.path.join(tmp, "ngps")
    os.makedirs(ddir), os.makedirs(sdir)
    names = ["img%d" % k for k in range(N)]
    for k, name in enumerate(names):
        os.makedirs(os.path.join(gdir, name))
        write_tiff_stack(os.path.join(gdir, name, name + ".tif"), g["gt_%d" % k])
        write_tiff_stack(os.path.join(ddir, name + ".tif"), g["dsn_%d" % k])
        with open(os.path.join(sdir, name + ".swc"), "wb") as f:
            f.write(g["swc_%d" % k].tobytes())
    return gdir, {"dsn": ddir, "ngps": sdir}, names


@pytest.mark.parametrize("flag", ["dsn", "ngps"])
def test_baseline_files_and_cli(g, flag, tmp_path):
    gdir, pdirs, names = baseline_tree(g, str(tmp_path))
    for t in sorted(TAGS):
        tag = "%s_%s" % (flag, TAGS[t])
        prec, rec = EB.calc_instance_segmentation_voc_prec_rec(flag.upper(), pdirs[flag], gdir, names, t)
        assert np.array_equal(bits(prec), bits(g[tag + "_prec"])) and np.array_equal(bits(rec), bits(g[tag + "_rec"]))
        res = EB.eval_instance_segmentation_soma(flag.upper(), pdirs[flag], gdir, names, t)
        assert bits(res["ap"]) == bits(g[tag + "_ap"]) and bits(res["map"]) == bits(g[tag + "_ap"])
        assert np.array_equal(bits(res["per_image_ap"]), bits(g[tag + "_per_image_ap"]))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "soma-" + flag, pdirs[flag], gdir, "--iou-thresh", "0.5"],
                         check=True, capture_output=True, text=True, timeout=600).stdout
    assert out.rstrip().split("\n")[-1] == "ap: {}".format(np.float64(g["%s_05_ap" % flag]))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "evaluate.py"), "soma-" + flag, pdirs[flag], gdir, "--names", "img2", "img0"],
                         check=True, capture_output=True, text=True, timeout=600).stdout
    p2 = [m3d.label_components(g["dsn_%d" % k])[0] if flag == "dsn" else m3d.paint_spheres(g["spheres_%d" % k], g["gt_%d" % k].shape)
          for k in (2, 0)]
    want = B.prec_rec([p.cpu().numpy() for p in p2], [g["gt_2"], g["gt_0"]], 0.3)[2]
    assert out.rstrip().split("\n")[-1] == "ap: {}".format(want)


def test_baseline_edge_cases():
    shape = (10, 30, 30)
    bg = np.zeros(shape, np.uint16)
    blob = bg.copy()
    blob[2:8, 5:20, 5:20] = 1                                        # 1350 voxels
    gt = bg.copy()
    gt[2:8, 5:20, 6:21] = 4
    # predictions but no GT ids in the image: rows are false positives, the per-image AP is NaN; another image supplies the GT
    prec, rec, per, ids = EB.baseline_prec_rec([blob, blob], [bg, gt], 0.5)
    assert prec.tolist() == [0.0, 0.5] and rec.tolist() == [0.0, 1.0] and np.isnan(per[0]) and per[1] == 1.0
    assert [i.tolist() for i in ids] == [[1], [1]]
    with pytest.raises(ValueError):                                  # no GT in any image
        EB.baseline_prec_rec([blob], [bg], 0.5)
    with pytest.raises(ValueError):                                  # no background in the prediction
        EB.baseline_prec_rec([np.ones(shape, np.uint16)], [gt], 0.5)
    small_bg = np.ones(shape, np.uint16)
    small_bg[0, 0, :29] = 0                                          # background present but below the size filter
    with pytest.raises(ValueError):
        EB.baseline_prec_rec([small_bg], [gt], 0.5)
    # no surviving prediction: the image only adds to n_pos
    prec, rec, per, ids = EB.baseline_prec_rec([bg, blob], [gt, gt], 0.5)
    assert prec.tolist() == [1.0] and rec.tolist() == [0.5] and np.isnan(per[0]) and ids[0].size == 0
    # a row below the threshold goes to the pooled list only: the per-image AP sees an empty table
    far = bg.copy()
    far[2:8, 5:20, 0:4] = 1                                          # 360 voxels, IoU 0 with the GT
    prec, rec, per, ids = EB.baseline_prec_rec([far], [gt], 0.5)
    assert prec.tolist() == [0.0] and rec.tolist() == [0.0] and per == [0.0]


def test_label_volume_tool(tmp_path):
    rng = np.random.RandomState(4)
    _, pred, _ = synth_label_pair((16, 48, 80), 7, 9)
    m = ((pred > 0) * 255).astype(np.uint8)
    m[rng.uniform(size=m.shape) < 0.003] = 255
    src, dst = str(tmp_path / "in.tif"), str(tmp_path / "out.tif")
    write_tiff_stack(src, m)
    tool = os.path.join(ROOT, "tools", "label_volume.py")
    out = subprocess.run([sys.executable, tool, src, dst, "--connectivity", "6"], check=True, capture_output=True, text=True, timeout=600).stdout
    want, k = ndimage.label(m, structure=ndimage.generate_binary_structure(3, 1))
    got = read_tiff_stack(dst)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    sizes = np.sort(np.bincount(want.ravel())[1:])[::-1][:5]
    assert out.split("\n")[0] == "K: %d" % k and out.split("\n")[1] == "largest: " + " ".join(str(v) for v in sizes)
    out = subprocess.run([sys.executable, tool, src, dst, "--min-voxels", "50"], check=True, capture_output=True, text=True, timeout=600).stdout
    want, k = ndimage.label(m, structure=np.ones((3, 3, 3), bool))
    cnt = np.bincount(want.ravel())
    keep = cnt >= 50
    keep[0] = False
    new = np.cumsum(keep) * keep
    assert np.array_equal(read_tiff_stack(dst), new[want].astype(np.uint16)) and out.split("\n")[0] == "K: %d" % keep.sum()
    # more components than uint16 holds: an error that names K
    V = 70000 * 2
    many = np.zeros((1, 1, V), np.uint8)
    many[0, 0, ::2] = 1
    write_tiff_stack(src, many)
    r = subprocess.run([sys.executable, tool, src, dst], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "70000" in r.stderr
