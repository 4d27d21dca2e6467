"""GPU: peak stimulation (csrc/peak_stim.hip, m3d/peaks.py) against the recorded results of the reference's function
(tests/golden/peak_stimulation.npz) and against the NumPy restatement of the contract (tests/peak_stimulation_reference.py); the
driver kwargs and the engine's stimulated tile on the smallest synthetic net of tests/test_gpu_prm.py.  Comparisons are exact unless
a bound is stated."""
import os

import numpy as np
import pytest
import torch

import peak_stimulation_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "peak_stimulation.npz")
TILE = (4, 4, 16)                      # outputs of one workgroup of the peak-map kernel (csrc/peak_stim.hip: TZ, TY, TX)
CHUNK = 1024                           # voxels of one workgroup of its count / compaction kernels


def golden_names():
    return [str(n) for n in np.load(GOLDEN)["names"]]


def device_filter(z, name, dev):
    kind = str(z[name + "_filter"])
    if kind == "none":
        return None
    if kind == "const":
        return float(z[name + "_value"])
    if kind == "tensor":                                                  # as the reference passes it: a callable giving [B,C,1,1,1]
        thr = torch.from_numpy(z[name + "_thresh"]).to(dev)
        return lambda t: thr.view(t.shape[0], t.shape[1], 1, 1, 1)
    return kind


def run_dev(x, win, filt, cap=None):
    import m3d
    out = m3d.peak_stimulation_3d_dev(x, win, filt, cap=cap)
    n = int(out["num"].item())
    return out, n


def check_against(x_np, win, filt_dev, filt_ref, what):
    """The whole op on x_np against the restatement: list, count, thresholds, aggregation, map - all exact."""
    x = torch.from_numpy(x_np).cuda()
    out, n = run_dev(x, win, filt_dev)
    ref = R.peak_stimulation(x_np, win, filt_ref)
    assert n == ref["peaks"].shape[0], (what, n, ref["peaks"].shape[0])
    assert np.array_equal(out["peaks"][:n].cpu().numpy(), ref["peaks"]), what
    assert np.array_equal(out["peak_map"].cpu().numpy().astype(bool), ref["peak_map"]), what
    assert np.array_equal(out["thresh"].cpu().numpy(), ref["thresh"], equal_nan=True), what
    assert np.array_equal(out["agg"].cpu().numpy(), ref["agg"], equal_nan=True), what
    return out, ref


def tied(rng, shape, levels=5):
    return (rng.randint(0, levels, shape) / 4.0 - 0.5).astype(np.float32)


@pytest.mark.parametrize("name", golden_names())
def test_golden_case(name):
    """Every recorded case of the reference: peaks, count, thresholds, aggregation (NaN positions included) and gx."""
    import m3d
    z = np.load(GOLDEN)
    x = torch.from_numpy(z[name + "_x"]).cuda().requires_grad_(True)
    win = int(z[name + "_win"])
    peaks, agg = m3d.peak_stimulation_3d(x, True, win, device_filter(z, name, x.device))
    assert peaks.dtype == torch.int64 and not peaks.requires_grad and agg.requires_grad
    assert peaks.shape == z[name + "_peaks"].shape and np.array_equal(peaks.cpu().numpy(), z[name + "_peaks"])
    assert np.array_equal(agg.detach().cpu().numpy(), z[name + "_agg"], equal_nan=True)
    (gx,) = torch.autograd.grad(agg, x, torch.from_numpy(z[name + "_gy"]).cuda())
    assert np.array_equal(gx.cpu().numpy(), z[name + "_gx"], equal_nan=True)
    out = m3d.peak_stimulation_3d_dev(x.detach(), win, device_filter(z, name, x.device))
    assert int(out["num"].item()) == z[name + "_peaks"].shape[0]
    assert np.array_equal(out["thresh"].cpu().numpy(), z[name + "_thresh"], equal_nan=True)
    only = m3d.peak_stimulation_3d(x.detach(), False, win, device_filter(z, name, x.device))                  # :40-41
    assert torch.is_tensor(only) and torch.equal(only, peaks)


SHAPES = [(TILE[0] + 1, TILE[1], TILE[2]), (TILE[0], TILE[1] + 1, TILE[2]), (TILE[0], TILE[1], TILE[2] + 1),   # one voxel past the tile
          (1, 1, 37), (9, 1, 1), (1, 7, 1),                                                                      # degenerate axes
          (4, 16, 16), (1, 25, 41), (3, 19, 37)]                                                                 # n = CHUNK, CHUNK + 1, 2 chunks + tail


@pytest.mark.parametrize("win", [1, 3, 5, 9])
def test_tile_edges_and_degenerate_axes(win):
    rng = np.random.RandomState(100 + win)
    for shp in SHAPES:
        for bc in ((1, 1), (2, 3)):
            x = tied(rng, bc + shp)
            check_against(x, win, None, None, (win, bc, shp))
            check_against(x, win, "median", "median", (win, bc, shp, "median"))


def test_all_equal_volume_has_one_peak_per_channel():
    for shp in ((2, 3, 5, 6, 17), (1, 2, 9, 9, 33)):
        for win in (3, 9):
            out, ref = check_against(np.full(shp, 0.25, np.float32), win, "max", "max", (shp, win))
            want = np.array([[b, c, 0, 0, 0] for b in range(shp[0]) for c in range(shp[1])])
            assert np.array_equal(ref["peaks"], want)
            assert np.array_equal(out["agg"].cpu().numpy(), np.full(shp[:2], 0.25, np.float32))


def test_nan_inf_and_negative_zero():
    """NaN beats everything (the last NaN of a window wins), 0 * NaN / 0 * inf poison the aggregation as in the reference, -0.0 ties with
    +0.0; -inf (outside the reference's contract) is the smallest ordinary value - an all -inf channel has its one peak at the origin."""
    rng = np.random.RandomState(5)
    x = tied(rng, (2, 3, 6, 7, 19), levels=3)
    x[x == 0] = rng.choice([0.0, -0.0], int((x == 0).sum())).astype(np.float32)
    x[0, 0, 2, 2, 2] = x[0, 0, 2, 3, 3] = x[0, 0, 5, 6, 18] = np.nan
    x[0, 1, 1, 1, 1] = np.inf
    x[0, 2, 3, 3, 3] = x[0, 2, 3, 3, 4] = np.inf
    x[1, 0] = -np.inf
    x[1, 1, 0, 0, 0] = x[1, 1, 5, 6, 18] = -np.inf
    for win in (3, 5):
        for filt in (None, 0.0, "median", "mean", "max"):
            out, ref = check_against(x, win, filt, filt, (win, filt))
        o, _ = check_against(x, win, None, None, win)
        rows = o["peaks"][:int(o["num"].item())].cpu().numpy()
        assert [r.tolist() for r in rows if r[0] == 1 and r[1] == 0] == [[1, 0, 0, 0, 0]]


def test_median_equals_torch_median():
    import m3d
    g = torch.Generator().manual_seed(3)
    for shp in ((2, 3, 5, 6, 7), (1, 2, 4, 4, 4), (1, 4, 7, 13, 31), (1, 1, 1, 1, 1), (1, 2, 1, 1, 2)):       # odd and even n, n > 1024
        x = torch.randn(shp, generator=g)
        x[x.abs() < 0.3] = 0.0                                               # many zeros, of both signs: the median of (0, 0) / (1, 0)
        x = torch.where((torch.rand(shp, generator=g) < 0.5) & (x == 0), torch.full_like(x, -0.0), x)
        if x.numel() > 50:
            x[0, 0] = x[0, 0].abs().neg()                                    # a negative channel
            x[0, 1].view(-1)[5] = float("nan")                              # torch.median: NaN if the channel holds one
        out = m3d.peak_stimulation_3d_dev(x.cuda(), 3, "median", cap=0)
        want = x.view(shp[0], shp[1], -1).median(2)[0]
        got = out["thresh"].cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(want))
        assert torch.equal(got[~torch.isnan(got)], want[~torch.isnan(want)])     # as values: -0.0 == +0.0


def test_mean_within_2_ulp_and_peaks_follow_the_device_threshold():
    import m3d
    g = torch.Generator().manual_seed(4)
    for shp in ((2, 3, 5, 6, 7), (1, 5, 7, 13, 31)):
        x = torch.randn(shp, generator=g) * 3 + 1
        out, n = run_dev(x.cuda(), 3, "mean")
        got = out["thresh"].cpu()
        want = x.view(shp[0], shp[1], -1).mean(2)
        ulp = torch.from_numpy(np.spacing(np.abs(want.numpy())))
        print("mean: max |device - torch.mean| / ulp = %.3f" % float(((got - want).abs() / ulp).max()))
        assert bool(((got - want).abs() <= 2 * ulp).all())
        exact = (x.double().view(shp[0], shp[1], -1).sum(2) / (shp[2] * shp[3] * shp[4])).float()          # fp64 sum, rounded once
        assert torch.equal(got, exact)
        ref = R.peak_stimulation(x.numpy(), 3, None, thresh=got.numpy())
        assert n == ref["peaks"].shape[0] and np.array_equal(out["peaks"][:n].cpu().numpy(), ref["peaks"])


def test_cap_below_the_count():
    import m3d
    rng = np.random.RandomState(9)
    x_np = tied(rng, (2, 3, 5, 9, 33))
    ref = R.peak_stimulation(x_np, 3, None)
    n = ref["peaks"].shape[0]
    cap = n // 2
    assert cap >= 8
    x = torch.from_numpy(x_np).cuda()
    L = m3d._lib.lib()
    B, C, S, H, W = x.shape
    import ctypes
    peaks = torch.full((cap + 1, 5), -7, dtype=torch.int32, device="cuda")          # row `cap` is the sentinel behind the list
    num = torch.zeros((1,), dtype=torch.int64, device="cuda")
    thr = torch.empty((B * C,), device="cuda")
    wsb = L.m3d_peak_stimulation3d_workspace_bytes(B, C, S, H, W, 3)
    ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda")
    rc = L.m3d_peak_stimulation3d(ctypes.c_void_p(x.data_ptr()), B, C, S, H, W, 3, 0, ctypes.c_float(0.0), None, None,
                                  ctypes.c_void_p(peaks.data_ptr()), cap, ctypes.c_void_p(num.data_ptr()), None,
                                  ctypes.c_void_p(thr.data_ptr()), None, ctypes.c_void_p(ws.data_ptr()), ctypes.c_size_t(wsb),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert int(num.item()) == n                                                      # the true count
    got = peaks.cpu().numpy()
    assert np.array_equal(got[:cap], ref["peaks"][:cap]) and (got[cap] == -7).all()
    # the synchronous form retries once with the true count when its buffer overflows
    from m3d import peaks as pk
    old = pk.DEFAULT_PEAK_CAP
    pk.DEFAULT_PEAK_CAP = cap
    try:
        full, _ = m3d.peak_stimulation_3d(x, True, 3, None)
    finally:
        pk.DEFAULT_PEAK_CAP = old
    assert np.array_equal(full.cpu().numpy(), ref["peaks"])


def test_soma_sized_map_and_bit_identical_reruns():
    import m3d
    from m3d.config import Cfg
    c = Cfg.soma()
    shp = (1, c.num_anchors) + tuple(v // c.stride for v in c.in_size)               # [1,14,16,40,40]
    g = torch.Generator().manual_seed(8)
    x = torch.sigmoid(torch.randn(shp, generator=g) * 4)                             # a response map: sigmoid outputs, some saturated
    out, ref = check_against(x.numpy(), 3, "median", "median", "soma")
    again = m3d.peak_stimulation_3d_dev(x.cuda(), 3, "median")
    n = int(out["num"].item())
    assert n > 1000
    for k in ("num", "thresh", "agg", "peak_map"):
        assert torch.equal(out[k], again[k]), k
    assert torch.equal(out["peaks"][:n], again["peaks"][:n])
    assert torch.equal(out["agg"].view(torch.int32), again["agg"].view(torch.int32))


def test_autograd_is_peak_map_times_gy():
    import m3d
    g = torch.Generator().manual_seed(12)
    x = torch.randn((2, 3, 5, 9, 21), generator=g).cuda().requires_grad_(True)
    peaks, agg = m3d.peak_stimulation_3d(x, win_size=5, peak_filter="mean")
    gy = torch.randn((2, 3), generator=g).cuda()
    (gx,) = torch.autograd.grad(agg, x, gy)
    pm = m3d.peak_stimulation_3d_dev(x.detach(), 5, "mean")["peak_map"]
    assert int(pm.sum().item()) == peaks.shape[0] > 0
    assert torch.equal(gx, pm.float() * gy.view(2, 3, 1, 1, 1))
    with pytest.raises(ValueError):
        m3d.peak_stimulation_3d(x, win_size=4)


# ------------------------------------------------------------------------------------------------ driver and engine
def _small_net():
    import oracle as O
    P = O.make_params(stride=8, num_anchors=35, mlp_dim=32, seed=2)
    cfg = O.Cfg(mlp_dim=32, score_thresh=0.0, in_size=(16, 24, 24), crop_ovlp=8)
    crop = np.random.RandomState(3).randn(16, 24, 24).astype(np.float32)
    return P, cfg, crop


def test_driver_returns_aggregation_and_maps():
    from m3d.drivers import PeakResponseMapping_3d
    P, cfg, crop = _small_net()
    model = PeakResponseMapping_3d(P, cfg, enable_peak_stimulation=True, enable_peak_backprop=False, win_size=3, filter_type="median")
    data = torch.from_numpy(np.stack([crop, crop[::-1].copy()])[:, None])            # a batch of two
    im_info = torch.tensor([[16, 24, 24, 1.0]], dtype=torch.float64)
    res = model(data=[data], im_info=[im_info], im_scale=[1.0])
    assert isinstance(res, tuple) and len(res) == 2
    agg, crm = res
    assert crm.is_cuda and crm.shape == (2, 35, 2, 3, 3) and agg.shape == (2, 35)
    ref = R.peak_stimulation(crm.cpu().numpy(), 3, "median")
    assert np.array_equal(agg.cpu().numpy(), ref["agg"], equal_nan=True)
    one = PeakResponseMapping_3d(P, cfg)(data=[data[:1]], im_info=[im_info], im_scale=[1.0])      # stimulation off: unchanged tuple
    assert len(one) == 5
    model.inferencing = False                                                        # :193
    only = model(data=[data], im_info=[im_info])
    assert torch.is_tensor(only) and torch.equal(only, agg)
    for kw in (dict(filter_type="mean"), dict(filter_type=0.5), dict(filter_type=None), dict(win_size=1)):
        m = PeakResponseMapping_3d(P, cfg, enable_peak_stimulation=True, enable_peak_backprop=False, **kw)
        a, c = m(data=[data[:1]], im_info=[im_info])
        filt = kw.get("filter_type", "median")
        r = R.peak_stimulation(c.cpu().numpy(), kw.get("win_size", 3), filt)
        if filt == "mean":
            r = R.peak_stimulation(c.cpu().numpy(), 3, None, thresh=m3d_thresh(c, "mean"))
        assert np.array_equal(a.cpu().numpy(), r["agg"], equal_nan=True), kw
    with pytest.raises(NotImplementedError, match="prm_tile_stimulated"):
        PeakResponseMapping_3d(P, cfg, enable_peak_stimulation=True)
    with pytest.raises(NotImplementedError, match="bilinear"):
        PeakResponseMapping_3d(P, cfg, enable_peak_stimulation=True, enable_peak_backprop=False, sub_pixel_locating_factor=2)


def m3d_thresh(crm, filt):
    import m3d
    return m3d.peak_stimulation_3d_dev(crm, 3, filt, cap=0)["thresh"].cpu().numpy()


def test_engine_stimulated_tile():
    from m3d.model import DetectorM3D
    from m3d.prm import PRMEngine
    P, cfg, crop = _small_net()
    eng = PRMEngine(DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg))
    data = torch.from_numpy(crop[None, None]).cuda()
    for filt, thr in (("median", 0.1), (None, 0.5), (0.3, 0.1)):
        out = eng.prm_tile_stimulated(data, peak_threshold=thr, win_size=3, peak_filter=filt, dense=True)
        crm = out["crm"].cpu().numpy()
        ref = R.peak_stimulation(crm, 3, filt)
        keep = crm[tuple(ref["peaks"].T)] > np.float32(thr)                          # each peak's own response (:158-162), list order
        want = ref["peaks"][keep]
        assert want.shape[0] > 0 and "dets" not in out
        assert out["peaks"].dtype == torch.int64 and np.array_equal(out["peaks"].cpu().numpy(), want)
        assert np.array_equal(out["peaks_dev"].cpu().numpy(), want[:, 1:])
        feat, prob, deltas, saved, top = eng.forward(data)
        assert torch.equal(prob, out["crm"])
        win, sums, origins = eng.backward_windows(out["peaks_dev"], saved, top, data)
        assert torch.equal(win, out["windows"]) and torch.equal(sums, out["sums"]) and torch.equal(origins, out["origins"])
        assert out["prms"].shape == (want.shape[0], 16, 24, 24) and out["num_live"] == want.shape[0]
    assert eng.prm_tile_stimulated(data, peak_threshold=2.0) is None                  # no response above 2: nothing is kept
