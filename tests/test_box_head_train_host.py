"""CPU: the NumPy restatement of the box-head training step (tests/box_head_train_reference.py) reproduces the reference's own results
(tests/golden/box_head_train.npz, made by gen_box_head_train.py from add_proposals, _sample_rois and fast_rcnn_losses): overlaps,
classes, assignments, sampled rows, labels, rois, counts, weights and dx,dy,dz bit for bit, dw,dh,ds within 4 fp32 ulp, losses and
gradients within the bounds of loss_bounds().  Plus: the sampling is uniform enough and without replacement, the C entry points
validate their arguments without a GPU, and the public wrappers refuse CPU tensors."""
import ctypes
import os

import numpy as np
import pytest

import box_head_train_reference as BR
from rpn_train_reference import stream

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "box_head_train.npz")
CASES = ["nuclei", "soma", "small_crowd", "small_fewfg", "small_short", "small_lo", "small_3cls"]
LOSS_CASES = {"loss_small2": ["small_crowd", "small_short"], "loss_nuclei": ["nuclei"]}
EPS = 2.0 ** -24
LOG_ULP = 4      # NumPy's fp32 log within 1 ulp, then an fp32 product: two relative errors of 2^-23 can reach 4 ulp of the result


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def case_inputs(g, name):
    """cfg, gt, classes, crowd, proposals, seed"""
    p = name + "_"
    n = g[p + "numbers"]
    cfg = BR.make_cfg(n[0], n[1], n[2], n[3], n[4], n[5], g[p + "weights"])
    return cfg, g[p + "gt"], g[p + "gt_classes"], g[p + "gt_crowd"], g[p + "proposals"], int(g[p + "seed"])


_memo = {}


def restated(g, name):
    """(labelling, sampled set) of a golden case, computed once and shared; callers must not change it"""
    if name not in _memo:
        cfg, gt, cls, crowd, pr, seed = case_inputs(g, name)
        L = BR.label(gt, pr, cls, crowd)
        _memo[name] = (L, BR.sample(L, cfg, seed))
    return _memo[name]


def ulp_distance(a, b):
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def loss_inputs(seed, N, C):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((N, C)) * 2).astype(np.float32), (rng.standard_normal((N, 6 * C)) * 1.5).astype(np.float32)


def compact_of(dense, labels):
    """[n, 6C] blob -> the six slots of each row's label (zeros for label <= 0)"""
    out = np.zeros((len(labels), 6), np.float32)
    for i in np.flatnonzero(np.asarray(labels) > 0):
        out[i] = dense[i, 6 * labels[i]:6 * labels[i] + 6]
    return out


def check_sampled(T, cfg, g, name, what=""):
    """a trimmed sampled set (dict of rows, labels, rois [n,6], targets [n,6] compact, counts) against the reference's blobs"""
    p = name + "_"
    assert np.array_equal(T["counts"], g[p + "counts"]), (T["counts"], g[p + "counts"])
    assert np.array_equal(T["rows"], g[p + "rows"]) and np.array_equal(T["labels"], g[p + "labels"])
    assert T["labels"].dtype == np.int32 and T["rows"].dtype == np.int64
    assert np.array_equal(bits(T["rois"]), bits(g[p + "rois"][:, 1:]))
    want = compact_of(g[p + "bbox_targets"], g[p + "labels"])
    tg = np.asarray(T["targets"], np.float32)
    assert tg.shape == want.shape
    assert np.array_equal(bits(tg[:, :3]), bits(want[:, :3]))
    d = ulp_distance(tg[:, 3:], want[:, 3:])
    print(name, what, "log targets: largest ulp distance", int(d.max()) if d.size else 0)
    assert (d <= LOG_ULP).all()
    assert (tg[T["labels"] <= 0] == 0).all()


def check_blobs(bt, iw, ow, g, name):
    p = name + "_"
    gt_, gi, go = g[p + "bbox_targets"], g[p + "inside"], g[p + "outside"]
    assert bt.dtype == iw.dtype == ow.dtype == np.float32 and bt.shape == gt_.shape
    assert np.array_equal(bits(iw), bits(gi)) and np.array_equal(bits(ow), bits(go))
    assert np.array_equal(bt != 0, gt_ != 0)
    comp = np.arange(bt.shape[1]) % 6
    assert np.array_equal(bits(bt[:, comp < 3]), bits(gt_[:, comp < 3]))
    assert (ulp_distance(bt[:, comp >= 3], gt_[:, comp >= 3]) <= LOG_ULP).all()


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(g, name):
    cfg = case_inputs(g, name)[0]
    L, T = restated(g, name)
    p = name + "_"
    assert np.array_equal(bits(L["overlap"]), bits(g[p + "max_overlaps"]))           # add_proposals / _add_class_assignments
    assert np.array_equal(L["cls"], g[p + "max_classes"]) and np.array_equal(L["assign"], g[p + "gt_map"])
    check_sampled(T, cfg, g, name)
    check_blobs(*BR.blobs(T, cfg), g, name)


def test_fixture_holds_the_cases_it_claims(g):
    c = {n: g[n + "_counts"] for n in CASES}
    for n, batch in (("nuclei", 64), ("soma", 128)):          # 2000 proposals, both sets sub-sampled
        assert c[n][7] == 2000 and c[n][0] == batch and c[n][1] == batch // 4 and c[n][3] > c[n][1] and c[n][4] > c[n][2]
    K = 6
    mo, gm, rows = g["small_crowd_max_overlaps"], g["small_crowd_gt_map"], g["small_crowd_rows"]
    crowd = int(np.flatnonzero(g["small_crowd_gt_crowd"])[0])
    assert c["small_crowd"][5] == 1 and mo[crowd] == -1 and crowd not in rows and not (gm[K:] == crowd).any()
    assert np.array_equal(g["small_crowd_gt"][2], g["small_crowd_gt"][3]) and (gm[K:] == 2).any() and not (gm[K:] == 3).any()
    assert (mo[K:] == 1).any()                                                       # a proposal identical to a box
    n_fg = c["small_crowd"][1]
    assert (rows[:n_fg] < K).any() and (rows[:n_fg] >= K).any()                      # a gt row among the sampled fg
    assert c["small_fewfg"][1] == c["small_fewfg"][3] < 16 and c["small_fewfg"][0] == 64
    assert c["small_short"][0] < 64 and c["small_short"][0] == c["small_short"][3] + c["small_short"][4]
    lo = g["small_lo_max_overlaps"]
    assert g["small_lo_numbers"][4] == 0.1 and ((lo > 0) & (lo < np.float32(0.1))).any() and c["small_lo"][3] + c["small_lo"][4] < len(lo)
    assert g["small_3cls_numbers"][5] == 3 and set(g["small_3cls_labels"][:c["small_3cls"][1]].tolist()) == {1, 2}
    assert os.path.getsize(GOLD) < 512 * 1024


def loss_case(g, lname):
    """padded fp32 inputs of a loss case: scores [B batch, C], predictions [B batch, 6C], labels [B batch] (-1 = padding), the
    reference's own compact targets [B batch, 6], and the cases' batch"""
    names = LOSS_CASES[lname]
    cfg = case_inputs(g, names[0])[0]
    batch, C = cfg["batch"], cfg["num_classes"]
    sc, pr = loss_inputs(int(g[lname + "_seed"]), len(names) * batch, C)
    labels, targets = np.full(len(names) * batch, -1, np.int32), np.zeros((len(names) * batch, 6), np.float32)
    for i, n in enumerate(names):
        lab = g[n + "_labels"]
        labels[i * batch:i * batch + len(lab)] = lab
        targets[i * batch:i * batch + len(lab)] = compact_of(g[n + "_bbox_targets"], lab)
    return sc, pr, labels, targets, batch


def loss_bounds(l64, gs64, gp64, R, n_fg):
    """How far the reference's fp32 results may lie from the fp64 evaluation of the same formulas on the same fp32 inputs.
    loss_cls is the fp32 mean of R non-negative terms, each a log-softmax good to a few ulp: worst-case summation of n positive terms
    is n 2^-24 relative, 8 more for the terms' own error and the divide.  loss_bbox sums 6 n_fg non-zero non-negative terms (the zeros
    of the dense blob add nothing), each a subtraction, a square or an abs, and two products: (6 n_fg + 8) 2^-24 relative.  The
    accuracy is an exact count divided once: 2^-24 relative.  A gradient element is a softmax value <= 1 good to a few ulp, one
    subtraction and one divide by R (for the box term a subtraction, a clamp and the divide): 8 2^-24 of max(|g|, 1/R)."""
    floor = 1.0 / R if R else 0.0
    return ((R + 8) * EPS * l64[0], (6 * n_fg + 8) * EPS * l64[1], EPS * l64[2], 8 * EPS * np.maximum(np.abs(gs64), floor),
            8 * EPS * np.maximum(np.abs(gp64), floor))


def check_losses_against_reference(losses, gs, gp, g, lname, what):
    """fp32 results (the reference's are the fixture's; a device's are passed in) against the fp64 restatement on the same inputs"""
    sc, pr, labels, targets, _ = loss_case(g, lname)
    lc, lb, acc, gs64, gp64, R = BR.losses(sc, pr, labels, targets, np.float64)
    bounds = loss_bounds((lc, lb, acc), gs64, gp64, R, int((labels > 0).sum()))
    ref = np.asarray(losses, np.float64)
    print(lname, what, "loss err", abs(ref[0] - lc), "of", bounds[0], "|", abs(ref[1] - lb), "of", bounds[1], "| acc", abs(ref[2] - acc))
    assert abs(ref[0] - lc) <= bounds[0] and abs(ref[1] - lb) <= bounds[1] and abs(ref[2] - acc) <= bounds[2]
    assert np.array_equal(gs != 0, gs64 != 0) and np.array_equal(gp != 0, gp64 != 0)
    assert (np.abs(gs - gs64) <= bounds[3]).all() and (np.abs(gp - gp64) <= bounds[4]).all()
    return (lc, lb, acc, gs64, gp64, R)


@pytest.mark.parametrize("lname", sorted(LOSS_CASES))
def test_reference_losses_lie_within_bounds_of_the_restatement(g, lname):
    check_losses_against_reference(g[lname + "_losses"], g[lname + "_grad_score"], g[lname + "_grad_pred"], g, lname, "reference")
    sc, pr, labels, targets, _ = loss_case(g, lname)
    d = np.abs(pr.reshape(len(labels), -1, 6)[np.flatnonzero(labels > 0), labels[labels > 0]] - targets[labels > 0])
    assert (d < 1).any() and (d >= 1).any()                      # both smooth-L1 branches
    srt = np.sort(sc, 1)
    assert (srt[:, 1:] != srt[:, :-1]).all()                     # no two scores of a row tie


@pytest.mark.ref
def test_live_generator_equals_committed_file(g):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD)))
    import ref_harness
    if not ref_harness.available():
        pytest.skip("reference tree not present")
    import gen_box_head_train
    live = gen_box_head_train.build_arrays()
    assert sorted(live) == sorted(g)
    for k in g:
        a, b = np.asarray(live[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def sampling_deviation(g, seeds):
    """Label small_crowd once, re-run only the sampling for each seed: the worst deviation, in binomial sigma, of a candidate's keep
    count from (rows kept / candidates), over the fg and the bg set."""
    cfg = case_inputs(g, "small_crowd")[0]
    L = restated(g, "small_crowd")[0]
    fgc, bgc = BR.candidates(L, cfg)
    n_fg = BR.fg_per_im(cfg)
    n_bg = cfg["batch"] - n_fg
    assert len(fgc) > n_fg and len(bgc) > n_bg
    keep = np.zeros(L["K"] + L["n"], np.int64)
    for seed in seeds:
        T = BR.sample(L, cfg, seed)
        assert len(np.unique(T["rows"])) == len(T["rows"]) == cfg["batch"]          # without replacement
        assert np.isin(T["rows"][:n_fg], fgc).all() and np.isin(T["rows"][n_fg:], bgc).all()
        assert (np.diff(T["rows"][:n_fg]) > 0).all() and (np.diff(T["rows"][n_fg:]) > 0).all()
        keep[T["rows"]] += 1
    worst = []
    for cand, k in ((fgc, n_fg), (bgc, n_bg)):
        p = k / len(cand)
        worst.append(np.abs(keep[cand] - len(seeds) * p).max() / np.sqrt(len(seeds) * p * (1 - p)))
    print("worst deviation: fg %.2f sigma, bg %.2f sigma" % tuple(worst))
    return worst


def test_sampling_is_uniform_over_2000_seeds(g):
    """Over seeds 0..1999 every fg candidate's keep count lies within 5 binomial sigma of fg_per_im / #fg candidates and every bg
    candidate's within 5 sigma of #bg kept / #bg candidates (measured: 2.69 and 2.56 sigma over 88 and 237 candidates; DESIGN)."""
    worst_fg, worst_bg = sampling_deviation(g, range(2000))
    assert worst_fg <= 5 and worst_bg <= 5


def test_base_seed_contract():
    """bg keys are taken 2^40 rows away from the fg keys in the same stream, and the stream is the finaliser of the seed"""
    cand = np.arange(10, dtype=np.int64)
    a = BR.choose(cand, 3, stream(5), 0)
    b = BR.choose(cand + (1 << 40), 3, stream(5), 0) - (1 << 40)
    assert np.array_equal(BR.choose(cand, 3, stream(5), 1 << 40), b) and len(a) == 3
    assert not np.array_equal(BR.choose(np.arange(1000), 100, stream(5), 0), BR.choose(np.arange(1000), 100, stream(6), 0))


def test_argument_validation_without_gpu():
    """The entry points reject bad arguments and the documented limits before they touch the device."""
    import __graft_entry__ as entry
    entry.build()
    from m3d._lib import LIB_PATH
    L = ctypes.CDLL(LIB_PATH)
    L.m3d_box_head_targets_workspace_bytes.restype = ctypes.c_size_t
    d = ctypes.c_double
    one = ctypes.c_void_p(256)     # never dereferenced: every call below fails validation first
    off = (ctypes.c_int32 * 3)(0, 4, 6)
    bad_off = (ctypes.c_int32 * 3)(0, 4, 3)
    seeds = (ctypes.c_uint64 * 2)(1, 2)
    wt = (d * 6)(10, 10, 10, 5, 5, 5)

    def targets(B=2, rows=100, batch=64, fg=16, C=2, agnostic=0, offp=off, seedp=seeds, wtp=wt, ws=one, gt=one, num=one):
        return L.m3d_box_head_targets(gt, None, None, offp, B, one, num, rows, batch, fg, d(0.4), d(0.4), d(0.0), wtp, C, agnostic, seedp,
                                      one, one, one, one, one, ws, ctypes.c_size_t(0), None)
    assert targets(B=0) == -1 and targets(rows=-1) == -1 and targets(batch=0, fg=0) == -1 and targets(fg=65) == -1 and targets(C=1) == -1
    assert targets(offp=None) == -1 and targets(seedp=None) == -1 and targets(wtp=None) == -1 and targets(offp=bad_off) == -1
    assert targets(ws=None) == -1 and targets(gt=None) == -1 and targets(num=None) == -1
    assert targets(C=65) == -4 and targets(batch=4097) == -4 and targets(B=65) == -4 and targets(agnostic=1) == -4   # the limits
    assert targets(rows=2 ** 31 - 200) == -4                                          # K + rows must stay below 2^31
    assert targets() == -3                                                            # workspace too small
    assert L.m3d_box_head_targets_workspace_bytes(2, 40, 2000) > 0 and L.m3d_box_head_targets_workspace_bytes(65, 40, 2000) == 0
    assert L.m3d_box_head_targets_workspace_bytes(2, 40, 2 ** 31 - 200) == 0
    blobs = L.m3d_box_head_target_blobs
    assert blobs(one, one, ctypes.c_int64(64), 2, None, one, one, None) == -1 and blobs(one, one, ctypes.c_int64(-1), 2, one, one, one, None) == -1
    assert blobs(one, one, ctypes.c_int64(64), 65, one, one, one, None) == -4
    loss = L.m3d_box_head_loss
    assert loss(one, one, one, one, one, 2, 64, 2, None, one, one, None) == -1 and loss(one, one, one, one, one, 0, 64, 2, one, one, one, None) == -1
    assert loss(one, one, one, one, one, 2, 64, 65, one, one, one, None) == -4 and loss(one, one, one, one, one, 2, 4097, 2, one, one, one, None) == -4


def test_no_cpu_fallback():
    import torch
    import m3d
    with pytest.raises(TypeError):
        m3d.BoxHeadTrainCfg.nuclei(batch_per_img=32)          # a misspelt key is an error, not a silent default
    n, s = m3d.BoxHeadTrainCfg.nuclei(), m3d.BoxHeadTrainCfg.soma()
    assert (n.batch_per_im, n.fg_per_im, s.batch_per_im, s.fg_per_im) == (64, 16, 128, 32)
    for c in (n, s):
        assert (c.fg_fraction, c.fg_thresh, c.bg_thresh_hi, c.bg_thresh_lo, c.num_classes) == (0.25, 0.4, 0.4, 0.0, 2)
        assert tuple(c.bbox_reg_weights) == (10, 10, 10, 5, 5, 5) and not c.cls_agnostic_bbox_reg
    rois, num = torch.zeros((1, 10, 7)), torch.zeros((1,), dtype=torch.int32)
    with pytest.raises(m3d.M3DError):
        m3d.box_head_targets(rois, num, [np.zeros((1, 6), np.float32)], n, seed=1)
    T = m3d.BoxHeadTargets(torch.zeros((1, 64), dtype=torch.int64), torch.zeros((1, 64), dtype=torch.int32), torch.zeros((1, 64, 6)),
                           torch.zeros((1, 64, 6)), torch.zeros((1, 8), dtype=torch.int64), n)
    with pytest.raises(m3d.M3DError):
        m3d.box_head_losses(torch.zeros((64, 2)), torch.zeros((64, 12)), T)
    with pytest.raises(m3d.M3DError):
        T.blobs()
