"""The detection box head as one library call (m3d_box_head_forward, DetectorM3D._box_head_call) against the per-layer path it replaces
on the bare path (the path that stays under a probe): cls, bbox and pred_boxes bit for bit, at row counts on each side of every plan
threshold of csrc/fc_gemm.hip (<= 32 rows: fp32-input GEMM; 128- / 256-row tiles around 256; the 256 x 256 tiles from 384 rows on),
with an empty batch item, on grown buffers whose stale rows hold NaN, and with the probe's spans still recorded."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FEAT = (2, 32, 4, 6, 6)
MLP = 256
ROWS = [0, 20, 33, 255, 257, 383, 385]


def make_rois(R, seed, empty_item=None):
    """[R, 7] (batch, x1, y1, z1, x2, y2, z2) in image voxels (stride 8: a 48 x 48 x 32 image); no row of item `empty_item`"""
    g = np.random.RandomState(seed)
    lim = np.array([FEAT[4], FEAT[3], FEAT[2]], np.float64) * 8
    lo = g.rand(R, 3) * (lim - 6)
    hi = np.minimum(lo + 2 + g.rand(R, 3) * lim * 0.6, lim - 1)
    b = g.randint(0, FEAT[0], (R, 1)).astype(np.float64)
    if empty_item is not None:
        b[:] = 1 - empty_item
    b = np.sort(b, axis=0)                                   # rows of one item are contiguous, as compact_rows leaves them
    return torch.from_numpy(np.hstack([b, lo, hi]).astype(np.float32)).cuda()


@pytest.fixture(scope="module")
def det():
    import m3d  # noqa: F401
    from m3d.config import Cfg
    from m3d.model import DetectorM3D
    from m3d.synth import make_params
    assert torch.cuda.is_available()
    P = make_params(stride=8, num_anchors=5, mlp_dim=MLP, seed=11)
    g = torch.Generator().manual_seed(12)
    K = FEAT[1] * 343
    P["Box_Head.fc1.weight"] = torch.randn(MLP, K, generator=g) * (2.0 / K) ** 0.5
    d = DetectorM3D({k: v.cuda() for k, v in P.items()}, Cfg.nuclei(mlp_dim=MLP))
    from m3d import ops
    assert all(isinstance(d.fc_split[n], ops.SplitLinearF16) for n in ("fc1", "fc2"))
    yield d
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def feat():
    return torch.randn(FEAT, generator=torch.Generator().manual_seed(5)).cuda().relu_()


def per_layer(det, feat, rois):
    """the path under a probe: one library call per layer"""
    from m3d.model import Probe
    det.probe = Probe()
    try:
        out = det.box_head_outputs(feat, rois, clip_to=(32., 48., 48.))
        return out, det.probe
    finally:
        det.probe = None


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("R", ROWS)
def test_one_call_equals_the_per_layer_path(det, feat, R):
    rois = make_rois(R, R + 1)
    want, _ = per_layer(det, feat, rois)
    got = det.box_head_outputs(feat, rois, clip_to=(32., 48., 48.))
    assert [tuple(t.shape) for t in got] == [(R, 2), (R, 12), (R, 12)]
    assert same(got, want)
    if R:
        assert bool(torch.isfinite(got[0]).all()) and float(got[0].sum(1).sub(1).abs().max()) < 1e-5
    assert (R > 32) == det._one_call_ok(feat, rois, R)       # <= 32 rows and no rows: the per-layer code on both sides


def test_the_feature_maps_bound_slots_give_the_same_bits(det, feat):
    """feat with the bound slots a conv leaves (its largest slot = max |feat|) and the zeroed fc1 -> fc2 row: nothing is swept, same bits"""
    from m3d import ops
    rois = make_rois(300, 3)
    want, _ = per_layer(det, feat, rois)
    for path in ("one call", "per layer"):
        f = feat.clone()
        slots = torch.zeros((2, ops.ZwConv3d.SLOTS), device="cuda")
        slots[0, 7] = feat.abs().max()
        slots[0, 9] = 0.5 * feat.abs().max()
        f._m3d_bound, f._m3d_head_bound = (slots[0], f._version), slots[1]
        got = per_layer(det, f, rois)[0] if path == "per layer" else det.box_head_outputs(f, rois, clip_to=(32., 48., 48.))
        assert same(got, want), path
        assert float(slots[1].max()) > 0 and "_m3d_head_bound" not in f.__dict__, path     # filled by fc1's storing launch, used once


def test_an_item_without_rois(det, feat):
    rois = make_rois(90, 4, empty_item=0)
    assert float(rois[:, 0].min()) == 1.0
    assert same(det.box_head_outputs(feat, rois, clip_to=(32., 48., 48.)), per_layer(det, feat, rois)[0])


def test_stale_rows_of_the_grown_buffers_are_not_read(det, feat):
    big, small = make_rois(385, 8), make_rois(131, 9)
    det.box_head_outputs(feat, big, clip_to=(32., 48., 48.))
    bufs = det._head_bufs[torch.cuda.current_stream().cuda_stream]
    assert bufs["rows"] >= 385
    for n in ("x", "h1", "h2", "outs"):
        bufs[n][131:].fill_(float("nan"))
    ptrs = bufs["ptrs"]
    got = det.box_head_outputs(feat, small, clip_to=(32., 48., 48.))
    assert det._head_bufs[torch.cuda.current_stream().cuda_stream]["ptrs"] == ptrs          # the same buffers: nothing was allocated
    assert same(got, per_layer(det, feat, small)[0])
    assert all(bool(torch.isnan(bufs[n][131:]).all()) for n in ("x", "h1", "h2", "outs"))   # ... and nothing written past the rows


def test_the_probe_still_gets_its_spans(det, feat):
    _, probe = per_layer(det, feat, make_rois(64, 2))
    torch.cuda.synchronize()
    ms = probe.median_ms()
    assert {"roi_align3d", "fc1", "fc2"} <= set(ms) and all(v > 0 for v in ms.values())


def test_detect_batch_takes_the_one_call_path_and_matches_the_probe_path():
    """end to end: detect_batch (bare: begin() prepares the call, finish() makes it) == the same step under a probe"""
    from m3d.config import Cfg
    from m3d.model import DetectorM3D, Probe
    from m3d.synth import make_params
    P = make_params(stride=8, num_anchors=35, mlp_dim=128, seed=3)
    det = DetectorM3D({k: v.cuda() for k, v in P.items()}, Cfg.nuclei(mlp_dim=128, score_thresh=0.0))
    vol = torch.randn((2, 1, 32, 64, 64), generator=torch.Generator().manual_seed(0)).cuda()
    bare = det.detect_batch(vol, as_dicts=False)
    assert sum(bare["num_rois"]) > 32 and "_head_bufs" in det.__dict__
    det.probe = Probe()
    probed = det.detect_batch(vol, as_dicts=False)
    assert {"roi_align3d", "fc1", "fc2"} <= set(det.probe.spans)
    for k in ("cls", "bbox", "pred_boxes", "cls_counts"):
        assert torch.equal(bare[k], probed[k]), k
    n = bare["cls_counts"].cpu().tolist()
    for b in range(2):
        for j in range(2):
            assert torch.equal(bare["cls_boxes"][b, j, :n[b][j]], probed["cls_boxes"][b, j, :n[b][j]]), (b, j)
