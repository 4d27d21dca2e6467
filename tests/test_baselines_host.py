"""CPU: the NumPy / SciPy restatement of the reference's baseline scoring script (tests/baseline_reference.py) reproduces the script's
own results (tests/golden/eval_baselines.npz, made by gen_eval_baselines.py) bit for bit, and the host parts of
m3d.evaluate_baselines - the size filter with its quirk, the SWC reader, the documented errors - match it.  No compute entry point
is called here (test_cabi.py: "no compute calls without a GPU")."""
import os

import numpy as np
import pytest

import baseline_reference as B
from m3d import evaluate_baselines as EB

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_baselines.npz")
TAGS = {0.3: "03", 0.5: "05", 0.7: "07"}
N = 3


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def swc_text(g, k):
    return g["swc_%d" % k].tobytes().decode("ascii")


def test_public_names():
    import m3d
    for name in ("label_components", "label_counts", "paint_spheres"):
        assert callable(getattr(m3d, name))
    for name in ("calc_instance_segmentation_voc_prec_rec", "eval_instance_segmentation_soma", "baseline_prec_rec", "read_swc_spheres",
                 "select_pred_ids"):
        assert callable(getattr(EB, name))


def test_select_pred_ids_worked_example():
    # ids 1 and 4 are removed, so 2 and 5 are never tested and survive with 20 and 5 voxels
    assert EB.select_pred_ids([0, 1, 2, 3, 4, 5], [10 ** 6, 10, 20, 500, 5, 5]) == [2, 3, 5]
    assert EB.select_pred_ids([0, 1, 2], [1000, 300, 299]) == [1]
    assert EB.select_pred_ids([0], [1000]) == []
    assert EB.select_pred_ids([0, 7], {0: 400, 7: 3}, min_voxels=4) == []


def test_select_pred_ids_errors():
    with pytest.raises(ValueError):
        EB.select_pred_ids([1, 2], [0, 500, 500])                 # no background at all
    with pytest.raises(ValueError):
        EB.select_pred_ids([0, 1, 2], [299, 500, 500])            # background below the size filter: removed, then remove(0) fails
    with pytest.raises(ValueError):
        EB.select_pred_ids([], [])


@pytest.mark.parametrize("k", range(N))
def test_select_pred_ids_matches_reference(g, k):
    dsn = B.label(g["dsn_%d" % k])[0]
    ngps = B.paint_spheres(g["spheres_%d" % k], g["gt_%d" % k].shape)
    for pred, key in ((dsn, "dsn_ids_%d" % k), (ngps, "ngps_ids_%d" % k)):
        cnt = np.bincount(pred.ravel().astype(np.int64))
        got = EB.select_pred_ids(np.nonzero(cnt > 0)[0], cnt)
        assert got == g[key].tolist() == B.select_ids(pred)
    # the quirk is in play: survivors below the size filter exist in the DSN images
    cnt = np.bincount(dsn.ravel().astype(np.int64))
    assert (cnt[g["dsn_ids_%d" % k]] < 300).any() and (cnt[g["dsn_ids_%d" % k]] >= 300).any()


@pytest.mark.parametrize("k", range(N))
def test_read_swc_spheres_matches_reference(g, k, tmp_path):
    p = tmp_path / "a.swc"
    p.write_text(swc_text(g, k))
    sp = EB.read_swc_spheres(str(p))
    assert sp.dtype == np.int64 and np.array_equal(sp, g["spheres_%d" % k]) and np.array_equal(sp, B.read_swc(swc_text(g, k)))
    # the fixture holds the cases it claims: a negative x that truncates toward zero, a radius below 6, a radius of at least 6 at the corner
    assert "-0.7" in swc_text(g, k) and (sp[:, 0] == 0).any() and (sp[:, 3] < 6).any()


def test_read_swc_truncates_toward_zero(tmp_path):
    p = tmp_path / "b.swc"
    p.write_text("1 1 -3.9 2.9 -0.2 6.99 -1\n2 1 1e1 7 8 9 1  \n")
    assert EB.read_swc_spheres(str(p)).tolist() == [[-3, 2, 0, 6], [10, 7, 8, 9]]


def test_read_swc_errors(tmp_path):
    p = tmp_path / "empty.swc"
    p.write_text("")
    with pytest.raises(ValueError):
        EB.read_swc_spheres(str(p))
    p.write_text("1 1 2 3\n")
    with pytest.raises(ValueError):
        EB.read_swc_spheres(str(p))


@pytest.mark.parametrize("flag", ["dsn", "ngps"])
@pytest.mark.parametrize("t", sorted(TAGS))
def test_restatement_matches_reference(g, flag, t):
    gts = [g["gt_%d" % k] for k in range(N)]
    if flag == "dsn":
        preds = [B.label(g["dsn_%d" % k])[0] for k in range(N)]
    else:
        preds = [B.paint_spheres(g["spheres_%d" % k], gts[k].shape) for k in range(N)]
    prec, rec, ap, per, ids = B.prec_rec(preds, gts, t)
    tag = "%s_%s" % (flag, TAGS[t])
    assert np.array_equal(bits(prec), bits(g[tag + "_prec"]))
    assert np.array_equal(bits(rec), bits(g[tag + "_rec"]))
    assert bits(ap) == bits(g[tag + "_ap"])
    assert np.array_equal(bits(per), bits(g[tag + "_per_image_ap"]))
    assert [list(i) for i in ids] == [g["%s_ids_%d" % (flag, k)].tolist() for k in range(N)]


def test_fixture_sphere_cases(g):
    """the clamp at index 1, the skipped id and the overwrite order are all visible in the painted volumes"""
    for k in range(N):
        sp = g["spheres_%d" % k]
        vol = B.paint_spheres(sp, g["gt_%d" % k].shape)
        n = len(sp)
        corner, small, over = n - 2, n - 1, n                     # ids of the three extra spheres
        assert (vol == corner).any() and not vol[0].any() and not vol[:, 0].any() and not vol[:, :, 0].any()
        assert (vol[1:, 1:, 1] == corner).any()                   # it would reach index 0 without the clamp
        assert sp[small - 1, 3] < 6 and not (vol == small).any()
        x, y, z, r = sp[0]
        zz, yy, xx = np.ogrid[:vol.shape[0], :vol.shape[1], :vol.shape[2]]
        both = ((xx - x) ** 2 + (yy - y) ** 2 + (zz - z) ** 2 <= r * r) & (vol == over)
        assert both.any()                                         # voxels of sphere 1 now carry the later id


def test_restatement_label_semantics():
    x = np.zeros((3, 4, 6), np.uint8)
    x[0, 0, 0:2] = 5
    x[0, 0, 2:4] = 9                                              # touches the 5s: a different value, a different component
    x[1, 1, 4] = 9                                                # diagonal to x[0, 0, 3] in all three axes
    lab26, k26 = B.label(x, 26)
    lab6, k6 = B.label(x, 6)
    assert k26 == 2 and lab26[0, 0, 0] == 1 and lab26[0, 0, 2] == 2 and lab26[1, 1, 4] == 2 and lab26[1, 1, 3] == 0
    assert k6 == 3 and lab6[1, 1, 4] == 3


def test_use_07_metric_raises_before_any_read():
    with pytest.raises(NotImplementedError):
        EB.eval_instance_segmentation_soma("DSN", "/nonexistent", "/nonexistent", ["a"], 0.3, use_07_metric=True)


def test_bad_flag():
    with pytest.raises(ValueError):
        EB.calc_instance_segmentation_voc_prec_rec("CPU", "/nonexistent", "/nonexistent", [], 0.3)
