"""GPU: training minibatches made on the device (csrc/train_sample.hip, m3d/data.py) against the NumPy restatement of
tests/train_sample_reference.py - all comparisons exact.  info, boxes, keep and score equal the restatement; data is bit-equal to
ops.norm1(vol, f32_arith=True) cropped at the origin.  Every output lies between sentinels that must keep their values."""
import os

import numpy as np
import pytest
import torch

import train_sample_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "train_sample.npz")
IN_SIZE = (8, 16, 12)
SENT = 16                                   # sentinel elements on either side of every output
SENT_F, SENT_I = -1234.5, 0x5a5a5a5a


@pytest.fixture(scope="module")
def m3d_gpu():
    import __graft_entry__ as g
    g.build()
    import m3d
    assert torch.cuda.is_available()
    return m3d


@pytest.fixture(scope="module")
def G():
    return dict(np.load(GOLD))


def int_boxes(rng, K, dims, lo=1, hi=9, corner=(0, 0, 0)):
    """K non-degenerate boxes with integer coordinates inside a volume (D, H, W), none below `corner` (x, y, z)"""
    D, H, W = dims
    out = np.zeros((0, 6), np.float32)
    while len(out) < K:
        n = 2 * K
        c = np.stack([rng.randint(0, W, n), rng.randint(0, H, n), rng.randint(0, D, n)], 1)
        r = rng.randint(lo, hi, (n, 3))
        b = np.concatenate([np.maximum(c - r, 0), np.minimum(c + r, np.array([W, H, D]) - 1)], 1).astype(np.float32)
        out = np.concatenate([out, b[(b[:, 3] > b[:, 0]) & (b[:, 4] > b[:, 1]) & (b[:, 5] > b[:, 2])]])
    out = out[:K]
    out[:, :3] = np.maximum(out[:, :3], np.array(corner, np.float32))
    out[:, 3:] = np.maximum(out[:, 3:], out[:, :3] + 1)
    return np.ascontiguousarray(out)


def volume(seed, dims, dtype=np.uint16):
    rng = np.random.RandomState(seed)
    v = rng.randint(0, 4000, dims)
    v[rng.uniform(size=dims) < 0.2] = 0                  # background voxels, outside the statistics
    return v.astype(dtype)


class Image:
    """a volume on the device with its statistics, its norm1 (the reference of `data`, computed once) and its boxes"""

    def __init__(self, m3d, vol, boxes):
        self.host, self.boxes_host = vol, np.ascontiguousarray(boxes, np.float32)
        self.dims = tuple(int(v) for v in vol.shape)
        self.vol = torch.from_numpy(vol).cuda()
        self.norm, self.stats_of_norm1 = m3d.norm1(self.vol, f32_arith=True, return_stats=True)
        self.stats = m3d.norm1_stats(self.vol)
        self.boxes = torch.from_numpy(self.boxes_host).cuda()

    def desc(self, in_size):
        return (self.vol, self.stats, self.boxes, R.start_max(self.boxes_host, self.dims, in_size))


def guarded(n, dtype, fill, shift=0):
    buf = torch.full((n + 2 * SENT + shift,), fill, dtype=dtype, device="cuda")
    return buf, buf[SENT + shift:SENT + shift + n]


def intact(buf, view, fill):
    h, n, at = buf.cpu().numpy(), view.numel(), view.storage_offset()
    return (h[:at] == fill).all() and (h[at + n:] == fill).all() and at >= SENT and len(h) - at - n >= SENT


def run(m3d, images, in_size, seeds, need_crop=True, fixed=None, max_boxes=None, shift=0):
    """one m3d_train_sample call with every output between sentinels -> (data tensor, dict of host arrays)"""
    B = len(images)
    M = max(len(im.boxes_host) for im in images) if max_boxes is None else max_boxes
    s, h, w = in_size
    bd, data = guarded(B * s * h * w, torch.float32, SENT_F, shift)
    bm, meta = guarded(B * (8 + M), torch.int32, SENT_I)
    bb, boxes = guarded(B * M * 6, torch.float32, SENT_F)
    bs, score = guarded(B, torch.float64, SENT_F)
    out = m3d.train_sample([im.desc(in_size) for im in images], in_size, need_crop, seeds, M, fixed_origin=fixed, data=data, meta=meta,
                           boxes_out=boxes, score=score)
    torch.cuda.synchronize()
    assert out[0].data_ptr() == data.data_ptr() and out[0].shape == (B, 1, s, h, w)
    assert intact(bd, data, np.float32(SENT_F)), "data sentinels"
    assert intact(bm, meta, SENT_I), "info / keep sentinels"
    assert intact(bb, boxes, np.float32(SENT_F)), "boxes sentinels"
    assert intact(bs, score, SENT_F), "score sentinels"
    return out[0], dict(boxes=out[1].cpu().numpy(), keep=out[2].cpu().numpy(), info=out[3].cpu().numpy(), score=out[4].cpu().numpy())


def check(m3d, images, in_size, seeds, need_crop=True, fixed=None, max_boxes=None, shift=0):
    data, got = run(m3d, images, in_size, seeds, need_crop, fixed, max_boxes, shift)
    M = got["keep"].shape[1]
    wants = []
    for b, im in enumerate(images):
        want = R.sample(im.boxes_host, im.dims, in_size, seeds[b], need_crop=need_crop, fixed_origin=None if fixed is None else fixed[b],
                        max_boxes=M)
        assert np.array_equal(got["info"][b], want["info"]), (b, got["info"][b], want["info"])
        assert np.array_equal(got["keep"][b], want["keep"]), b
        assert np.array_equal(got["boxes"][b].view(np.uint32), want["boxes"].view(np.uint32)), b
        assert got["score"][b] == want["score"], (b, got["score"][b], want["score"])
        x, y, z = want["origin"]
        ref = im.norm[z:z + in_size[0], y:y + in_size[1], x:x + in_size[2]]
        assert torch.equal(data[b, 0].view(torch.int32), ref.contiguous().view(torch.int32)), "data of image %d at %s" % (b, (x, y, z))
        wants.append(want)
    return data, got, wants


def three_boxes(rng, dims):
    """no box near the volume's low corner: start_max > 0 wherever the volume leaves room, so the seeds move the grid"""
    return [int_boxes(rng, k, d, corner=(4, 5, 3)) for d, k in zip(dims, (9, 4, 12))]


@pytest.fixture(scope="module")
def three(m3d_gpu):
    rng = np.random.RandomState(5)
    dims = [(20, 40, 30), (8, 50, 13), (30, 17, 40)]
    return [Image(m3d_gpu, volume(10 + i, d), b) for i, (d, b) in enumerate(zip(dims, three_boxes(rng, dims)))]


# ---------------------------------------------------------------------------------------------------------------- the search and the crop
def test_three_images_twenty_seeds(m3d_gpu, three):
    origins, dropped = set(), 0
    for seed in range(20):
        _, got, wants = check(m3d_gpu, three, IN_SIZE, [3 * seed, 3 * seed + 1, 3 * seed + 2])
        origins |= {(b,) + tuple(w["origin"]) for b, w in enumerate(wants)}
        dropped += sum(int(w["info"][3]) < len(im.boxes_host) for w, im in zip(wants, three))
        assert (got["info"][:, 4] == 0).all() and (got["info"][:, 5] > 1).all()
    assert len(origins) >= 10 and dropped > 0              # the seeds move the crop, and crops drop boxes


def test_volume_equals_in_size_and_no_crop(m3d_gpu, G):
    rng = np.random.RandomState(6)
    im = Image(m3d_gpu, volume(20, IN_SIZE), int_boxes(rng, 5, IN_SIZE))
    data, got, _ = check(m3d_gpu, [im], IN_SIZE, [1])
    assert torch.equal(data[0, 0], im.norm) and tuple(got["info"][0, :3]) == (0, 0, 0) and got["info"][0, 5] == 1
    # the nuclei yaml: boxes untouched, degenerate ones included
    im = Image(m3d_gpu, volume(21, IN_SIZE), G["nocrop_boxes"])
    data, got, _ = check(m3d_gpu, [im, im], IN_SIZE, [1, 2], need_crop=False)
    assert torch.equal(data[1, 0], im.norm) and np.array_equal(got["boxes"][0], G["nocrop_boxes"]) and list(got["keep"][1]) == [0, 1]
    assert tuple(got["info"][0]) == (0, 0, 0, 2, 0, 0, 0, 0) and got["score"][0] == 0.0


@pytest.mark.parametrize("name", ["tie", "drop", "draw3", "axis0", "full"])
def test_golden_cases(m3d_gpu, G, name):
    dims = tuple(int(v) for v in G[name + "_dims"])
    im = Image(m3d_gpu, volume(30, dims), G[name + "_boxes"])
    _, got, _ = check(m3d_gpu, [im], IN_SIZE, [int(G[name + "_seed"])])
    k = len(G[name + "_keep"])
    assert tuple(got["info"][0, :4]) == tuple(int(v) for v in G[name + "_origin"]) + (k,)
    assert np.array_equal(got["keep"][0, :k], G[name + "_keep"]) and np.array_equal(got["boxes"][0, :k], G[name + "_kept_boxes"])
    # classes and crowd flags follow keep (m3d.TrainSet)
    ts = m3d_gpu.TrainSet([im.host], [(G[name + "_boxes"], G[name + "_classes"], G[name + "_crowd"])], m3d_gpu.SampleCfg.soma(IN_SIZE=IN_SIZE, IM_SIZE=dims))
    batch = ts.sample([0], [int(G[name + "_seed"])])
    assert np.array_equal(batch.gt_classes[0], G[name + "_kept_classes"]) and np.array_equal(batch.gt_crowd[0], G[name + "_kept_crowd"])
    assert np.array_equal(batch.gt_boxes[0].cpu().numpy(), G[name + "_kept_boxes"]) and len(batch.gt_boxes) == 1
    gt, dc = batch.rpn_boxes(0)
    kc = G[name + "_kept_crowd"]
    assert np.array_equal(gt.cpu().numpy(), G[name + "_kept_boxes"][~kc]) and np.array_equal(dc.cpu().numpy(), G[name + "_kept_boxes"][kc])


def test_all_degenerate_boxes_and_fixed_origin(m3d_gpu, three):
    dims = (20, 40, 30)
    flat = np.array([[3, 4, 5, 3, 9, 8], [10, 12, 2, 15, 12, 6]], np.float32)         # no extent on x / on y: nothing scores above 0
    im = Image(m3d_gpu, volume(31, dims), flat)
    _, got, wants = check(m3d_gpu, [im], IN_SIZE, [6])
    assert got["info"][0, 4] == 1 and got["info"][0, 3] == 0 and got["score"][0] == 0.0 and (got["keep"][0] == -1).all()
    st = R.draw_starts(6, R.start_max(flat, dims, IN_SIZE))
    assert tuple(got["info"][0, :3]) == st and min(st) > 0  # the first candidate: the drawn start itself
    fixed = [(7, 3, 11), (1, 34, 0), (28, 0, 22)]          # odd ox on uint16; the last origin of an axis
    _, got, _ = check(m3d_gpu, three, IN_SIZE, [0, 0, 0], fixed=fixed)
    assert [tuple(r[:3]) for r in got["info"]] == fixed and (got["info"][:, 5] == 1).all()
    _, got, _ = check(m3d_gpu, [im], IN_SIZE, [0], fixed=[(2, 2, 2)])
    assert got["info"][0, 4] == 1


# ---------------------------------------------------------------------------------------------------------------- the store paths
@pytest.mark.parametrize("width,src,shift", [(9, np.uint16, 0), (12, np.uint16, 0), (12, np.uint16, 1), (9, np.float32, 0), (12, np.float32, 1),
                                             (16, np.uint16, 3)])
def test_store_paths(m3d_gpu, width, src, shift):
    """width 9: no row but the first starts on a 16-byte boundary; width 12: every row does - unless d_data is a view `shift` elements
    into a larger buffer.  Both source types, origins with an odd and an even ox."""
    rng = np.random.RandomState(width)
    dims, in_size = (11, 21, 29), (8, 16, width)
    vol = volume(40 + width, dims, src)
    if src == np.float32:
        vol = (vol * np.float32(0.37)).astype(np.float32)
    ims = [Image(m3d_gpu, vol, int_boxes(rng, 6, dims)) for _ in range(2)]
    last = 29 - width
    check(m3d_gpu, ims, in_size, [0, 0], fixed=[(min(5, last), 3, 1), (min(6, last), 5, 3)], shift=shift)
    check(m3d_gpu, ims, in_size, [8, 9], shift=shift)


# ---------------------------------------------------------------------------------------------------------------- the size limits
def test_one_box_and_2048_boxes(m3d_gpu):
    dims = (20, 40, 30)
    vol = volume(50, dims)
    rng = np.random.RandomState(51)
    one = Image(m3d_gpu, vol, int_boxes(rng, 1, dims))
    check(m3d_gpu, [one], IN_SIZE, [3])
    check(m3d_gpu, [one], IN_SIZE, [3], max_boxes=5)       # rows beyond the count: zeros and -1
    many = Image(m3d_gpu, vol, int_boxes(rng, 2048, dims, lo=1, hi=4))
    _, got, _ = check(m3d_gpu, [many, one], IN_SIZE, [5, 6])
    assert 0 < got["info"][0, 3] < 2048 and got["info"][1, 3] <= 1


def test_more_than_1024_candidates(m3d_gpu):
    dims, in_size = (12, 12, 12), (2, 2, 2)
    rng = np.random.RandomState(52)
    b = int_boxes(rng, 7, dims, lo=1, hi=3, corner=(1, 1, 1))
    b[0] = [1, 1, 1, 3, 3, 3]                              # start_max = 1: the grid starts at 0 or 1 on every axis
    im = Image(m3d_gpu, volume(53, dims), b)
    for seed in range(4):
        _, got, _ = check(m3d_gpu, [im], in_size, [seed])
        assert got["info"][0, 5] >= 1000                    # 10 candidates on an axis from start 1, 11 from start 0
    _, got, _ = check(m3d_gpu, [im], in_size, [R_seed_with_zero_starts(im, in_size)])
    assert got["info"][0, 5] == 1331


def R_seed_with_zero_starts(im, in_size):
    sm = R.start_max(im.boxes_host, im.dims, in_size)
    for seed in range(4096):
        if R.draw_starts(seed, sm) == (0, 0, 0):
            return seed
    raise AssertionError("no seed draws (0, 0, 0) from %s" % (sm,))


# ---------------------------------------------------------------------------------------------------------------- statistics
def test_norm1_stats_equal_norm1(m3d_gpu, three):
    for im in three:
        assert torch.equal(im.stats.view(torch.int64), im.stats_of_norm1.view(torch.int64)) and im.stats.shape == (3,)
        m = im.host[im.host > 0].astype(np.float64)
        assert im.stats[2].item() == len(m) and abs(im.stats[0].item() - m.mean()) < 1e-9 * m.mean()
    for dtype in (np.uint16, np.float32):
        vols = np.stack([volume(60 + i, (9, 17, 23), dtype) for i in range(3)])
        if dtype == np.float32:
            vols = vols * np.float32(0.61)
        dev = torch.from_numpy(vols).cuda()
        got = m3d_gpu.norm1_stats(dev, batch=3)
        assert got.shape == (3, 3)
        for i in range(3):
            _, single = m3d_gpu.norm1(dev[i], return_stats=True)
            assert torch.equal(got[i].view(torch.int64), single.view(torch.int64)), (dtype, i)
            assert torch.equal(m3d_gpu.norm1_stats(dev[i]).view(torch.int64), single.view(torch.int64))


def test_two_runs_are_bit_identical(m3d_gpu, three):
    a_data, a = run(m3d_gpu, three, IN_SIZE, [7, 8, 9])
    b_data, b = run(m3d_gpu, three, IN_SIZE, [7, 8, 9])
    assert torch.equal(a_data.view(torch.int32), b_data.view(torch.int32))
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------------------------------------------------------- m3d.TrainSet
def small_set(m3d, n=5, in_size=IN_SIZE):
    rng = np.random.RandomState(70)
    dims = [(int(rng.randint(in_size[0], in_size[0] + 14)), int(rng.randint(in_size[1], in_size[1] + 20)), int(rng.randint(in_size[2], in_size[2] + 20)))
            for _ in range(n)]
    vols = [volume(71 + i, d) for i, d in enumerate(dims)]
    anns = []
    for i, d in enumerate(dims):
        b = int_boxes(rng, 3 + i, d, lo=2, hi=max(4, in_size[0] // 2))
        anns.append((b, np.ones(len(b), np.int32), np.arange(len(b)) % 4 == 3))
    return m3d.TrainSet(vols, anns, m3d.SampleCfg.soma(IN_SIZE=in_size)), vols, anns, dims


def test_prefetch_yields_the_same_batches(m3d_gpu):
    ts, vols, anns, dims = small_set(m3d_gpu)
    plain = list(ts.batches(7, seed=3, prefetch=0))
    ahead = list(ts.batches(7, seed=3, prefetch=1))
    want_idx = R.batch_indices(len(ts), 2, 7, 3)
    assert len(plain) == len(ahead) == 7
    torch.cuda.synchronize()
    for t, (p, a) in enumerate(zip(plain, ahead)):
        assert p.indices == a.indices == want_idx[t]
        for x, y in ((p.data, a.data), (p.boxes, a.boxes), (p.keep, a.keep), (p.info, a.info), (p.score, a.score)):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        seeds = R.batch_seeds(3, t, 2)
        for b, i in enumerate(p.indices):
            want = R.sample(anns[i][0], dims[i], IN_SIZE, seeds[b], max_boxes=ts.max_boxes)
            assert np.array_equal(a.info[b].cpu().numpy(), want["info"]) and np.array_equal(a.host_info[b], want["info"])
            k = int(want["info"][3])
            assert np.array_equal(a.gt_boxes[b].cpu().numpy(), want["boxes"][:k])
            assert np.array_equal(a.gt_classes[b], anns[i][1][want["keep"][:k]]) and np.array_equal(a.gt_crowd[b], anns[i][2][want["keep"][:k]])


def test_hand_off_to_rpn_targets(m3d_gpu):
    in_size = (32, 64, 48)
    ts, vols, anns, dims = small_set(m3d_gpu, n=2, in_size=in_size)
    batch = ts.sample([0, 1], [11, 12])
    cfg = m3d_gpu.RpnTrainCfg(max_size=64)
    for b in range(2):
        want = R.sample(anns[b][0], dims[b], in_size, 11 + b)
        k = int(want["info"][3])
        crowd = anns[b][2][want["keep"][:k]]
        assert k > 0
        gt, dc_dev = batch.rpn_boxes(b)
        a = m3d_gpu.rpn_targets(gt, in_size, cfg, 5, dc_boxes=dc_dev).numpy()
        dc = want["boxes"][:k][crowd]
        w = m3d_gpu.rpn_targets(want["boxes"][:k][~crowd], in_size, cfg, 5, dc_boxes=dc if len(dc) else None).numpy()
        for key in a:
            assert a[key].tobytes() == w[key].tobytes(), key
    assert len(batch.gt_boxes) == len(batch.gt_classes) == len(batch.gt_crowd) == 2 and batch.gt_boxes[0].is_cuda
