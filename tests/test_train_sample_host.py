"""Training samples, the part that needs no GPU (DESIGN, "Training samples"): the NumPy restatement against the golden vectors made
from the reference's own prep_im_for_blob / crop_data_3d and dataset readers (tests/golden/gen_train_sample.py), m3d/data.py's readers and
epoch order against the restatement, the draws of the sampling contract, and every limit of m3d_train_sample - all of them refused before
a device pointer is followed."""
import ctypes as C

import numpy as np
import pytest

import train_sample_reference as R

EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


@pytest.fixture(scope="module")
def G(golden):
    return golden("train_sample")


def names_of(G):
    return bytes(G["names"]).decode().split(",")


# ---------------------------------------------------------------------------------------------------------------- 1. restatement == golden
def test_restatement_equals_the_reference(G):
    in_size = tuple(int(v) for v in G["in_size"])
    names = names_of(G)
    assert {"draw3", "axis0", "drop", "tie", "full", "nocrop"} <= set(names) and len(names) >= 12
    for n in names:
        dims = tuple(int(v) for v in G[n + "_dims"])
        got = R.sample(G[n + "_boxes"], dims, in_size, int(G[n + "_seed"]), need_crop=bool(G[n + "_need_crop"]))
        k = int(got["info"][3])
        assert tuple(got["origin"]) == tuple(int(v) for v in G[n + "_origin"]), n
        assert k == len(G[n + "_keep"]) and np.array_equal(got["keep"][:k], G[n + "_keep"]), n
        assert np.array_equal(got["boxes"][:k], G[n + "_kept_boxes"]) and got["boxes"].dtype == np.float32, n
        assert np.array_equal(G[n + "_classes"][got["keep"][:k]], G[n + "_kept_classes"]), n
        assert np.array_equal(G[n + "_crowd"][got["keep"][:k]], G[n + "_kept_crowd"]), n
        assert R.start_max(G[n + "_boxes"], dims, in_size) == tuple(int(v) for v in G[n + "_start_max"]), n
        assert got["score"] == G[n + "_score"] and int(got["info"][4]) == 0, n


def test_golden_cases_hold_what_they_exist_for(G):
    in_size = tuple(int(v) for v in G["in_size"])
    assert all(v > 0 for v in G["draw3_start_max"])
    assert G["axis0_start_max"][0] == 0 and G["axis0_start_max"][1] > 0
    assert len(G["drop_keep"]) < len(G["drop_boxes"])
    dims = tuple(int(v) for v in G["tie_dims"])
    sc = R.search(G["tie_boxes"], R.candidates((0, 0, 0), dims, in_size), in_size)[3]
    assert sc[0] == max(sc) and sc.count(max(sc)) == 2 and tuple(G["tie_origin"]) == (0, 0, 0)
    assert tuple(G["full_dims"]) == in_size
    assert int(G["nocrop_need_crop"]) == 0 and np.array_equal(G["nocrop_kept_boxes"], G["nocrop_boxes"])


@pytest.mark.ref
def test_live_generator_equals_committed_file(G):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import ref_harness
    if not ref_harness.available():
        pytest.skip("reference tree not present")
    import gen_train_sample
    live = gen_train_sample.build_arrays()
    assert sorted(live) == sorted(G.files)
    for k in G.files:
        a, b = np.asarray(live[k]), G[k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), k


def lines_of(a):
    return bytes(a).decode().splitlines(keepends=True)


def test_readers_equal_the_reference(G):
    import m3d
    lines = lines_of(G["soma_text"])
    im_size, ratio = tuple(int(v) for v in G["soma_im_size"]), float(G["soma_ratio"])
    b, c, cr, sg, v = R.read_soma(lines, im_size, ratio)
    a = m3d.read_soma_annotations(lines, m3d.SampleCfg.soma(IM_SIZE=im_size, RADIUS_EXP_RATIO=ratio))
    for got in ((b, c, cr, sg, v), (a.boxes, a.classes, a.crowd, a.segms, a.volumes)):
        for x, name in zip(got, ("boxes", "classes", "crowd", "segms", "volumes")):
            assert np.array_equal(x, G["soma_" + name]) and x.dtype == G["soma_" + name].dtype, name
    assert len(b) == len(lines) - 2                          # the soma of radius 0 is gone
    for n in ("nuc_mixed", "nuc_last"):
        lines, im_size = lines_of(G[n + "_text"]), tuple(int(v) for v in G[n + "_im_size"])
        r = R.read_nuclei(lines, G[n + "_mask"], im_size)
        a = m3d.read_nuclei_annotations(lines, G[n + "_mask"], m3d.SampleCfg.nuclei(IM_SIZE=im_size))
        for got in (r, (a.boxes, a.classes, a.crowd, a.volumes)):
            for x, name in zip(got, ("boxes", "classes", "crowd", "volumes")):
                assert np.array_equal(x, G["%s_%s" % (n, name)]) and x.dtype == G["%s_%s" % (n, name)].dtype, (n, name)
    assert list(G["nuc_last_crowd"]) == [True, True, False]              # the "last line" rule
    assert list(G["nuc_mixed_crowd"]) == [False, True, True, False, True]


def test_readers_read_files(tmp_path, G):
    import m3d
    p = tmp_path / "a.txt"
    p.write_bytes(bytes(G["soma_text"]))
    im_size = tuple(int(v) for v in G["soma_im_size"])
    a = m3d.read_soma_annotations(str(p), m3d.SampleCfg.soma(IM_SIZE=im_size, RADIUS_EXP_RATIO=float(G["soma_ratio"])))
    assert np.array_equal(a.boxes, G["soma_boxes"])
    boxes, classes, crowd, segms = a
    assert segms is a.segms and len(classes) == len(crowd) == len(boxes)


def test_cfg():
    import m3d
    n, s = m3d.SampleCfg.nuclei(), m3d.SampleCfg.soma()
    assert (n.PP_METHOD, n.NEED_CROP, n.IN_SIZE, n.IM_SIZE, n.RADIUS_EXP_RATIO, n.IMS_PER_BATCH) == ("norm1", False, (64, 256, 256), (64, 256, 256), 0.3, 2)
    assert (s.PP_METHOD, s.NEED_CROP, s.IN_SIZE, s.IM_SIZE, s.RADIUS_EXP_RATIO, s.IMS_PER_BATCH) == ("norm1", True, (64, 256, 256), (128, 256, 256), 0.2, 2)
    assert m3d.SampleCfg.soma(IN_SIZE=[8, 16, 12]).IN_SIZE == (8, 16, 12)
    with pytest.raises(ValueError):
        m3d.SampleCfg.nuclei(PP_METHOD="norm2")
    with pytest.raises(TypeError):
        m3d.SampleCfg.nuclei(USE_FLIPPED=True)


# ---------------------------------------------------------------------------------------------------------------- 2. the draws
def test_draws_cover_the_range():
    seen = [set(), set(), set()]
    for seed in range(64):
        st = R.draw_starts(seed, (3, 3, 3))
        for a in range(3):
            assert 0 <= st[a] <= 3
            seen[a].add(st[a])
    assert all(s == {0, 1, 2, 3} for s in seen)
    assert R.draw_starts(5, (0, 9, 0))[0] == 0 and R.draw_starts(5, (0, 9, 0))[2] == 0


def test_consecutive_seeds_are_unrelated():
    # without the stream scramble, axis a of seed s would be axis a - 1 of seed s + 1
    big = (1 << 20, 1 << 20, 1 << 20)
    draws = [R.draw_starts(s, big) for s in range(256)]
    shifted = sum(draws[s][1] == draws[s + 1][0] for s in range(255)) + sum(draws[s][2] == draws[s + 1][1] for s in range(255))
    assert shifted == 0
    assert len({d for d in draws}) == 256
    x = np.array([d[0] for d in draws], np.float64) / big[0]
    assert abs(np.corrcoef(x[:-1], x[1:])[0, 1]) < 0.25      # 255 pairs of independent uniforms: |r| beyond 4 sigma = 4 / sqrt(255)


def test_epoch_order():
    import m3d
    for n in (1, 2, 7, 50):
        for seed in (0, 1, 2 ** 63 + 5):
            for epoch in (0, 1, 5):
                o = m3d.epoch_order(n, seed, epoch)
                assert sorted(o) == list(range(n))
                assert o == m3d.epoch_order(n, seed, epoch) == [int(v) for v in R.epoch_order(n, seed, epoch)]
    orders = {tuple(m3d.epoch_order(50, s, e)) for s in range(4) for e in range(4)}
    assert len(orders) == 16                                 # another seed or another epoch: another order
    plan = R.batch_indices(7, 2, 8, 3)
    assert len(plan) == 8 and all(len(b) == 2 for b in plan)
    assert sorted(sum(plan[:3], [])) == sorted(int(v) for v in R.epoch_order(7, 3, 0)[:6])     # drop_last: 3 batches of epoch 0
    assert plan[3] == [int(v) for v in R.epoch_order(7, 3, 1)[:2]]


# ---------------------------------------------------------------------------------------------------------------- 3. the ABI's limits
def call(L, images, count=None, in_size=(8, 16, 12), need_crop=1, seeds=True, fixed=None, max_boxes=8, outs=None, query=True):
    """images: (vol, stats, boxes, dtype, (D, H, W), K, start_max).  With query=True a call that passes every check stores the
    workspace size and returns 0 without launching; nothing here ever reaches a launch."""
    from m3d._lib import TrainImage
    arr = (TrainImage * max(len(images), 1))()
    for e, (vol, stats, boxes, dtype, dims, K, sm) in zip(arr, images):
        e.vol, e.stats, e.boxes, e.dtype, e.num_boxes = vol, stats, boxes, dtype, K
        e.depth, e.height, e.width = dims
        e.start_max[0], e.start_max[1], e.start_max[2] = sm
    n = len(images) if count is None else count
    size = (C.c_int * 3)(*in_size) if in_size is not None else None
    sd = (C.c_uint64 * max(n, 1))(*range(max(n, 1))) if seeds else None
    fx = (C.c_int * (3 * len(fixed)))(*[v for o in fixed for v in o]) if fixed is not None else None
    o = [0x100000, 0x200000, 0x300000, 0x400000, 0x500000] if outs is None else outs
    need = C.c_size_t(99)
    rc = L.m3d_train_sample(arr if images else None, n, size, need_crop, sd, fx, max_boxes, C.c_void_p(o[0]), C.c_void_p(o[1]),
                            C.c_void_p(o[2]), C.c_void_p(o[3]), C.c_void_p(o[4]), None, C.byref(need) if query else None, None)
    if rc == 0 and query and n > 0:
        assert need.value == 0
    return rc


def test_abi_limits_without_a_gpu(L):
    from m3d._lib import SYMBOLS
    for s in ("m3d_train_sample", "m3d_norm1_stats"):
        assert s in SYMBOLS and hasattr(L, s), s
    ok = (0x10000, 0x20000, 0x30000, 0, (20, 40, 30), 3, (5, 7, 3))

    def im(**kw):
        d = dict(vol=ok[0], stats=ok[1], boxes=ok[2], dtype=ok[3], dims=ok[4], K=ok[5], sm=ok[6])
        d.update(kw)
        return (d["vol"], d["stats"], d["boxes"], d["dtype"], d["dims"], d["K"], d["sm"])
    assert call(L, [ok]) == 0 and call(L, [ok, ok]) == 0                         # the baseline passes every check
    assert call(L, [ok], count=-1) == EINVAL                                     # count < 0
    for bad in (dict(vol=None), dict(stats=None), dict(boxes=None)):             # null pointers
        assert call(L, [im(**bad)]) == EINVAL, bad
    assert call(L, [], count=1) == EINVAL and call(L, [ok], in_size=None) == EINVAL
    assert call(L, [ok], seeds=False) == EINVAL                                  # a search without seeds
    for k in range(5):
        outs = [0x100000, 0x200000, 0x300000, 0x400000, 0x500000]
        outs[k] = 0
        assert call(L, [ok], outs=outs) == EINVAL, k
        outs[k] = 0x100000 + (4 if k == 4 else 2)                                # d_score: 8-byte aligned, the others 4
        assert call(L, [ok], outs=outs) == EINVAL, k
    assert call(L, [im(vol=0x10001)]) == EINVAL                                  # uint16 volume on an odd address
    assert call(L, [im(vol=0x10002)]) == 0 and call(L, [im(vol=0x10002, dtype=1)]) == EINVAL
    assert call(L, [im(stats=0x20004)]) == EINVAL and call(L, [im(boxes=0x30002)]) == EINVAL
    assert call(L, [im(dtype=2)]) == EINVAL
    assert call(L, [im(dims=(7, 40, 30))]) == EINVAL and call(L, [im(dims=(20, 15, 30))]) == EINVAL and call(L, [im(dims=(20, 40, 11))]) == EINVAL
    for size in ((1, 16, 12), (8, 1, 12), (8, 16, 1), (0, 16, 12), (8, 16, -3)):  # an in_size entry < 2
        assert call(L, [ok], in_size=size) == EINVAL, size
    assert call(L, [ok], in_size=(2, 2, 2)) == 0
    for sm in ((-1, 7, 3), (5, -1, 3), (5, 7, -1), (19, 7, 3), (5, 25, 3), (5, 7, 13)):      # start_max outside [0, dim - size]
        assert call(L, [im(sm=sm)]) == EINVAL, sm
    assert call(L, [im(sm=(18, 24, 12))]) == 0
    for fx in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (19, 0, 0), (0, 25, 0), (0, 0, 13)):      # fixed_origin outside [0, dim - size]
        assert call(L, [ok], fixed=[fx]) == EINVAL, fx
    assert call(L, [ok], fixed=[(18, 24, 12)], seeds=False) == 0
    assert call(L, [ok], need_crop=0) == EINVAL                                  # no crop, but the volume is not IN_SIZE
    assert call(L, [im(dims=(8, 16, 12), sm=(0, 0, 0))], need_crop=0, seeds=False) == 0
    assert call(L, [im(K=0)]) == EINVAL and call(L, [im(K=-4)]) == EINVAL        # np.min of nothing
    assert call(L, [ok] * 64) == 0 and call(L, [ok] * 65) == EUNSUPPORTED        # count > 64
    assert call(L, [im(K=2048)], max_boxes=2048) == 0 and call(L, [im(K=2049)], max_boxes=4096) == EUNSUPPORTED
    assert call(L, [im(K=3)], max_boxes=2) == EUNSUPPORTED                       # max_boxes < K
    assert call(L, [im(dims=(4000, 4000, 4000), sm=(0, 0, 0))], in_size=(2, 2, 2)) == EUNSUPPORTED      # 2^31 candidates or more
    # count == 0: nothing to do, whatever else is passed; without the size query too - the runtime is not touched
    assert call(L, [], count=0) == 0 and call(L, [], count=0, query=False, outs=[0] * 5, in_size=None) == 0


def test_norm1_stats_refusals_without_a_gpu(L):
    f = L.m3d_norm1_stats
    ws = L.m3d_norm1_workspace_bytes()
    args = lambda **kw: [kw.get("d_in", C.c_void_p(0x10000)), kw.get("dtype", 0), kw.get("batch", 2), C.c_int64(kw.get("n", 100)),  # noqa: E731
                         kw.get("stats", C.c_void_p(0x20000)), kw.get("ws", C.c_void_p(0x30000)), C.c_size_t(kw.get("wsb", 2 * ws)), None]
    assert f(*args(d_in=None)) == EINVAL and f(*args(stats=None)) == EINVAL and f(*args(ws=None)) == EINVAL
    assert f(*args(n=0)) == EINVAL and f(*args(batch=0)) == EINVAL and f(*args(stats=C.c_void_p(0x20004))) == EINVAL
    assert f(*args(wsb=2 * ws - 1)) == -3


def test_no_cpu_path(L):
    import m3d
    import torch
    with pytest.raises(m3d.M3DError):
        m3d.norm1_stats(torch.zeros(8, 8, 8))
    with pytest.raises(m3d.M3DError):
        m3d.train_sample([(torch.zeros(8, 16, 12), torch.zeros(3, dtype=torch.float64), torch.zeros(1, 6), (0, 0, 0))], (8, 16, 12), True, [0], 1)
