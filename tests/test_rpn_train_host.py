"""CPU: the NumPy restatement of the RPN training step (tests/rpn_train_reference.py) reproduces the reference's own results
(tests/golden/rpn_train.npz, made by gen_rpn_train.py from _get_rpn_blobs and single_scale_rpn_losses): labels, index sets, weights
and dx,dy,dz bit for bit, dw,dh,ds within 2 fp32 ulp (NumPy's fp32 log is within 1 ulp of the true value, an fp64 log rounded once
within 0.5), losses and gradients within the bounds of loss_bounds().  Plus: the sampling hash is uniform enough, the C entry points
validate their arguments without a GPU, and the public wrappers refuse CPU tensors."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import rpn_train_reference as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rpn_train.npz")
CASES = ["nuclei", "soma", "small_all", "small_outside", "small_dc", "small_nobg"]
DENSE = CASES[2:]
LOSS_CASES = {"loss_nuclei": ["nuclei"], "loss_soma": ["soma"], "loss_small2": ["small_all", "small_outside"]}
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def case_inputs(g, name):
    p = name + "_"
    nums = g[p + "numbers"]
    cfg = R.make_cfg(nums[0], g[p + "sizes"], g[p + "aspect_ratios"], nums[1], nums[2], nums[3], nums[4], nums[5], nums[6], nums[7])
    return cfg, g[p + "gt"], g[p + "dc"], tuple(int(v) for v in g[p + "im_size"]), int(g[p + "seed"])


_memo = {}


def restated(g, name):
    if name not in _memo:
        cfg, gt, dc, im, seed = case_inputs(g, name)
        _memo[name] = R.rpn_targets(gt, im, cfg, seed, dc if len(dc) else None)
    return _memo[name]


def ulp_distance(a, b):
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


def loss_inputs(seed, B, A, s, h, w):
    rng = np.random.RandomState(seed)
    return ((rng.standard_normal((B, A, s, h, w)) * 2).astype(np.float32), (rng.standard_normal((B, 6 * A, s, h, w)) * 0.5).astype(np.float32))


def loss_bounds(l64, gl64, gp64, W, B, batch):
    """The loss sums <= B * batch non-negative fp32 terms: worst-case fp32 summation of n positive terms is n 2^-24 relative, 4 more
    for the few-ulp error of each term's exp / log1p.  A gradient element is sigmoid(x) to a few ulp on a value <= 1, then one
    subtraction and one divide (likewise one subtraction, a divide and a clamp for the box term): 8 2^-24 of max(|g|, 1/W)."""
    floor = 1.0 / W if W else 0.0
    return ((B * batch + 4) * EPS * l64[0], (B * batch + 4) * EPS * l64[1], 8 * EPS * np.maximum(np.abs(gl64), floor),
            8 * EPS * np.maximum(np.abs(gp64), floor))


def check_targets(T, g, name):
    p = name + "_"
    assert np.array_equal(T["fg_index"], g[p + "fg_index"]) and np.array_equal(T["bg_index"], g[p + "bg_index"])
    assert np.array_equal(T["target_index"], g[p + "target_index"])
    c, gc = T["counts"], g[p + "counts"]
    assert np.array_equal(c[:6], gc[:6])
    if gc[6] >= 0:          # the reference names the number of candidates only when it draws
        assert c[6] == gc[6] and c[7] == gc[7]
    else:
        assert c[7] == 0
    tg, gg = np.asarray(T["targets"], np.float32), g[p + "targets"]
    assert tg.shape == gg.shape
    assert np.array_equal(tg[:, :3].view(np.uint32), gg[:, :3].view(np.uint32))
    d = ulp_distance(tg[:, 3:], gg[:, 3:])
    print(name, "log targets: max ulp distance", int(d.max()) if d.size else 0)
    assert (d <= 2).all()


def check_wide(blobs, g, name):
    p = name + "_"
    lab, tw, iw, ow = blobs
    assert lab.dtype == np.int32 and tw.dtype == iw.dtype == ow.dtype == np.float32
    assert np.array_equal(sha(lab), g[p + "sha_labels"]) and np.array_equal(sha(iw), g[p + "sha_inside"])
    assert np.array_equal(sha(ow), g[p + "sha_outside"])
    if p + "labels_wide" in g:
        assert np.array_equal(lab, g[p + "labels_wide"]) and np.array_equal(iw.view(np.uint32), g[p + "inside_wide"].view(np.uint32))
        assert np.array_equal(ow.view(np.uint32), g[p + "outside_wide"].view(np.uint32))
        gt = g[p + "targets_wide"]
        A = lab.shape[1]
        comp = np.arange(6 * A) % 6
        assert np.array_equal(tw[:, comp < 3].view(np.uint32), gt[:, comp < 3].view(np.uint32))
        assert (ulp_distance(tw[:, comp >= 3], gt[:, comp >= 3]) <= 2).all()
        assert np.array_equal(tw != 0, gt != 0)


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(g, name):
    T = restated(g, name)
    check_targets(T, g, name)
    check_wide(R.wide(T), g, name)


def test_fixture_holds_the_cases_it_claims(g):
    c = {n: g[n + "_counts"] for n in CASES}
    assert tuple(c["nuclei"][[4, 5, 2, 6]]) == (119820, 89, 32, 119751) and tuple(c["soma"][[4, 5, 2, 6]]) == (491608, 1836, 64, 471243)
    assert c["small_all"][1] < c["small_all"][7]                                   # duplicate draws collapse
    assert c["small_outside"][5] == c["small_outside"][4] and c["small_outside"][0] < c["small_outside"][2]   # all fg; fg -> bg flips
    assert g["small_dc_dc"].size and c["small_nobg"][1] == 0 and c["small_nobg"][7] == 0


@pytest.mark.parametrize("lname", sorted(LOSS_CASES))
def test_restatement_losses_match_reference(g, lname):
    names = LOSS_CASES[lname]
    Ts = []
    for n in names:                       # the same fp32 inputs as the reference had: its own target rows
        T = dict(restated(g, n))
        T["targets"] = g[n + "_targets"]
        Ts.append(T)
    cfg, _, _, im, _ = case_inputs(g, names[0])
    st = cfg["stride"]
    lg, pr = loss_inputs(int(g[lname + "_seed"]), len(names), Ts[0]["A"], im[0] // st, im[1] // st, im[2] // st)
    lc, lb, gl, gp, W = R.losses(lg, pr, Ts, np.float64)
    bc, bb, bgl, bgp = loss_bounds((lc, lb), gl, gp, W, len(names), cfg["batch"])
    ref = g[lname + "_losses"].astype(np.float64)
    print(lname, "loss err", abs(ref[0] - lc), "of", bc, "|", abs(ref[1] - lb), "of", bb)
    assert abs(ref[0] - lc) <= bc and abs(ref[1] - lb) <= bb
    rgl, rgp = g[lname + "_grad_logits"], g[lname + "_grad_pred"]
    assert np.array_equal(rgl != 0, gl != 0) and np.array_equal(rgp != 0, gp != 0)
    assert (np.abs(rgl - gl) <= bgl).all() and (np.abs(rgp - gp) <= bgp).all()


@pytest.mark.ref
def test_live_generator_equals_committed_file(g):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLD)))
    import ref_harness
    if not ref_harness.available():
        pytest.skip("reference tree not present")
    import gen_rpn_train
    live = gen_rpn_train.build_arrays()
    assert sorted(live) == sorted(g)
    for k in g:
        a, b = np.asarray(live[k]), g[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def sampling_deviation(g, seeds):
    """Label once, re-run only the sampling for each seed: the worst deviation, in binomial sigma, of a fg anchor's keep count from
    num_fg / #fg and of a bg candidate's hit count from draws / n."""
    cfg, gt, dc, im, _ = case_inputs(g, "small_outside")
    L = R.label(gt, None, im, cfg)
    n_seeds, batch = len(seeds), cfg["batch"]
    num_fg = int(cfg["fg_fraction"] * batch)
    fld = L["inside"][np.where(L["fg"])[0]]
    n_fg, n = len(fld), int(L["cand"].sum())
    assert n_fg > num_fg and n > batch - num_fg
    keep, hits = np.zeros(n_fg, np.int64), np.zeros(n, np.int64)
    j = np.arange(batch - num_fg, dtype=np.uint64) + np.uint64(1 << 40)
    fg_wide, cand_wide = R.wide_index(L, fld), R.wide_index(L, L["inside"][np.where(L["cand"])[0]])
    for seed in seeds:
        st = R.stream(seed)
        order = np.lexsort((fld, R.key(st, fld)))
        keep[order[:num_fg]] += 1
        r = (R.key(st, j) * np.uint64(n)) >> np.uint64(32)
        np.add.at(hits, r.astype(np.int64), 1)
        T = R.sample(L, cfg, seed)           # the restatement's own sampling code draws exactly these sets
        assert np.array_equal(T["target_index"], np.sort(fg_wide[order[:num_fg]]))
        assert np.array_equal(T["bg_index"], np.unique(cand_wide[r.astype(np.int64)]))
        assert np.array_equal(T["fg_index"], np.setdiff1d(T["target_index"], T["bg_index"]))
    p = num_fg / n_fg
    worst_fg = np.abs(keep - n_seeds * p).max() / np.sqrt(n_seeds * p * (1 - p))
    trials, q = n_seeds * (batch - num_fg), 1.0 / n
    worst_bg = np.abs(hits - trials * q).max() / np.sqrt(trials * q * (1 - q))
    print("worst deviation: fg %.2f sigma, bg %.2f sigma" % (worst_fg, worst_bg))
    return worst_fg, worst_bg


def test_sampling_is_uniform_over_2000_seeds(g):
    """Over seeds 0..1999 every bg candidate's hit count lies within 5 binomial sigma of draws / n, and every fg anchor's keep count
    within 5 sigma of num_fg / #fg.  (Keys taken on seed + i directly, without the seed's stream, miss this: consecutive seeds then
    replay each other's draws shifted by one, and a candidate's hit count deviates by 19 sigma.)"""
    worst_fg, worst_bg = sampling_deviation(g, range(2000))
    assert worst_fg <= 5 and worst_bg <= 5


def test_key_is_the_documented_hash():
    # splitmix64's first outputs for state 0 are the finaliser of 1 * gamma, 2 * gamma, ...: key(0, 1) is the top half of the first
    assert int(R.key(0, 1)) == 0xE220A8397B1DCDAF >> 32 and int(R.key(1, 1)) == 0x6E789E6AA1B965F4 >> 32
    # a seed's stream is the whole finaliser of the seed: stream(1) is that first output, and consecutive seeds are far apart
    assert R.stream(1) == 0xE220A8397B1DCDAF and R.stream(2) == 0x6E789E6AA1B965F4 and R.stream(0) == 0


def test_argument_validation_without_gpu():
    """The four entry points reject bad arguments before they touch the device."""
    import __graft_entry__ as entry
    entry.build()
    from m3d._lib import LIB_PATH
    L = ctypes.CDLL(LIB_PATH)
    L.m3d_rpn_targets_workspace_bytes.restype = ctypes.c_size_t
    d = ctypes.c_double
    cell = (d * 12)(*range(12))
    one = ctypes.c_void_p(256)     # never dereferenced: every call below fails validation first

    def targets(A=2, F=8, stride=8, batch=64, num_fg=32, ws=one, cellp=cell, K=0):
        return L.m3d_rpn_targets(cellp, A, F, stride, None, K, None, 0, d(32), d(64), d(48), d(0), d(0.5), d(0.3), batch, num_fg,
                                 ctypes.c_uint64(1), one, one, one, one, one, ws, ctypes.c_size_t(0), None)
    assert targets(A=0) == -1 and targets(F=0) == -1 and targets(stride=0) == -1 and targets(cellp=None) == -1
    assert targets(num_fg=65) == -1 and targets(batch=0, num_fg=0) == -1 and targets(ws=None) == -1 and targets(K=3) == -1
    assert targets(A=65) == -4 and targets(batch=4097, num_fg=32) == -4 and targets(F=1024, A=8) == -4
    assert targets() == -3                                                           # workspace too small
    assert L.m3d_rpn_targets_workspace_bytes(2, 8, 0, 64, 32) > 0 and L.m3d_rpn_targets_workspace_bytes(65, 8, 0, 64, 32) == 0
    assert L.m3d_rpn_targets_wide(one, one, one, one, one, 2, 8, 32, 64, None, one, one, one, None) == -1
    assert L.m3d_rpn_targets_wide(one, one, one, one, one, 65, 8, 32, 64, one, one, one, one, None) == -4
    assert L.m3d_rpn_loss(one, one, 1, 2, 4, 8, 6, 8, one, one, one, one, one, 32, 64, None, one, one, None) == -1
    assert L.m3d_rpn_loss(one, one, 1, 2, 9, 8, 6, 8, one, one, one, one, one, 32, 64, one, one, one, None) == -1   # crop outside the field
    assert L.m3d_rpn_loss(one, one, 0, 2, 4, 8, 6, 8, one, one, one, one, one, 32, 64, one, one, one, None) == -1


def test_no_cpu_fallback():
    import torch
    import m3d
    with pytest.raises(TypeError):
        m3d.RpnTrainCfg.nuclei(batch_per_img=32)          # a misspelt key is an error, not a silent default
    cfg = m3d.RpnTrainCfg.nuclei(max_size=64)
    assert cfg.field_size == 8 and cfg.num_anchors == 35 and cfg.num_fg == 32
    assert m3d.RpnTrainCfg.soma().field_size == 64 and m3d.RpnTrainCfg.nuclei().field_size == 32
    with pytest.raises(m3d.M3DError):
        m3d.rpn_targets(torch.zeros((1, 6)), (32, 64, 48), cfg, seed=1)
