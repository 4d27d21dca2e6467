"""GPU parity tests: the HIP path (through the C ABI, include/m3d.h) against the CPU oracle and the golden
fixtures generated from the reference.  Bit-exact for integer/index work; fp32 conv within 1e-4 relative."""
import numpy as np
import pytest
import torch

import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    return _m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ NMS
def test_nms_golden_bit_exact(m3d, golden):
    g = golden("nms")
    for i in range(int(g["ncases"])):
        dets, thr = g["dets%d" % i], float(g["thr%d" % i])
        assert np.array_equal(m3d.nms3d(dev(dets), thr).cpu().numpy(), g["keep%d" % i]), i
        if "keepvol%d" % i in g:
            assert np.array_equal(m3d.nms3d(dev(dets), thr, by_volume=True).cpu().numpy(), g["keepvol%d" % i]), i


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 3000, 9000])
def test_nms_vs_oracle_random_and_ties(m3d, n):
    rs = np.random.RandomState(n)
    c = rs.uniform(0, 100, (n, 3)); s = rs.uniform(4, 40, (n, 3))
    b = np.hstack((c - s / 2, c + s / 2))
    sc = np.round(rs.uniform(0, 1, n), 2)            # many exact score ties -> exercises the tie rule
    dets = np.hstack((b, sc[:, None])).astype(np.float32)
    for thr in (0.15, 0.5):
        assert np.array_equal(m3d.nms3d(dev(dets), thr).cpu().numpy(), O.nms_3d(dets, thr))
    assert np.array_equal(m3d.nms3d(dev(dets), 0.3, by_volume=True).cpu().numpy(), O.nms_3d_volume(dets, 0.3))


@pytest.mark.parametrize("n,ext,thr_vol", [(16385, 140, 0.3), (17408, 140, 0.3), (17409, 140, 0.3), (20000, 150, 0.3), (50000, 200, 0.3),
                                           (100000, 250, 0.1)])
def test_nms_beyond_one_workgroups_capacity_equals_the_oracle(m3d, n, ext, thr_vol):
    """Cross-tile NMS has no bound on its row count (tools/binarization_nuclei.py:81, binarization_soma.py:57, lib/core/test.py:159):
    above 16 384 boxes m3d_nms3d runs the blocked form (chunks of 1024 sorted rows, csrc/box_ops.hip).  Same tie rule, same fp32
    IoU, bit-equal keep lists against the oracle in score order and in volume order; sizes on and around chunk edges."""
    rs = np.random.RandomState(n)
    c = rs.uniform(0, ext, (n, 3)); s = rs.uniform(4, 40, (n, 3))
    b = np.hstack((c - s / 2, c + s / 2))
    sc = np.round(rs.uniform(0, 1, n), 3)            # ~n / 1000 rows per distinct score: the tie rule decides thousands of visits
    dets = np.hstack((b, sc[:, None])).astype(np.float32)
    dets[rs.randint(0, n, 50)] = dets[rs.randint(0, n, 50)]          # exact duplicates (IoU 1, equal score: descending index wins)
    k = m3d.nms3d(dev(dets), 0.15).cpu().numpy()
    assert np.array_equal(k, O.nms_3d(dets, 0.15))
    assert np.array_equal(m3d.nms3d(dev(dets), thr_vol, by_volume=True).cpu().numpy(), O.nms_3d_volume(dets, thr_vol))
    k2 = m3d.nms3d(dev(dets[k]), 0.15).cpu().numpy()                 # idempotence: survivors do not suppress each other
    assert np.array_equal(k2, np.arange(len(k)))


def test_nms_blocked_form_extremes(m3d):
    """20 000 identical boxes -> exactly one survivor (the last row: ties visit the highest index first); 20 000 disjoint boxes ->
    all survive, in input order; the entry point refuses more than 2^20 rows instead of running for minutes."""
    n = 20000
    same = np.tile(np.array([[1, 2, 3, 11, 12, 13, 0.5]], np.float32), (n, 1))
    assert np.array_equal(m3d.nms3d(dev(same), 0.5).cpu().numpy(), [n - 1])
    assert np.array_equal(m3d.nms3d(dev(same), 0.5, by_volume=True).cpu().numpy(), [n - 1])
    g = np.arange(n)
    far = np.stack([(g % 100) * 20, (g // 100 % 100) * 20, (g // 10000) * 20], 1).astype(np.float32)
    rs = np.random.RandomState(3)
    dets = np.hstack((far, far + 9, rs.permutation(n)[:, None] / n)).astype(np.float32)
    assert np.array_equal(m3d.nms3d(dev(dets), 0.01).cpu().numpy(), g)
    import ctypes as C
    L = m3d._lib.lib()
    big = (1 << 20) + 1
    keep = torch.empty((8,), dtype=torch.int64, device="cuda"); num = torch.zeros((1,), dtype=torch.int32, device="cuda")
    rc = L.m3d_nms3d(C.c_void_p(keep.data_ptr()), big, C.c_float(0.3), 0, C.c_void_p(keep.data_ptr()), C.c_void_p(num.data_ptr()),
                     C.c_void_p(keep.data_ptr()), C.c_size_t(64), None)
    assert rc == -4                                                   # M3D_EUNSUPPORTED, before anything is launched


def test_nms_empty_and_idempotent(m3d):
    assert m3d.nms3d(torch.zeros((0, 7), device="cuda"), 0.3).numel() == 0
    rs = np.random.RandomState(5)
    c = rs.uniform(0, 60, (500, 3)); s = rs.uniform(4, 30, (500, 3))
    dets = np.hstack((c - s / 2, c + s / 2, rs.permutation(500)[:, None] / 500.)).astype(np.float32)
    k1 = m3d.nms3d(dev(dets), 0.2).cpu().numpy()
    k2 = m3d.nms3d(dev(dets[k1]), 0.2).cpu().numpy()
    assert np.array_equal(k2, np.arange(len(k1)))       # survivors do not suppress each other


# ------------------------------------------------------------------ IoU / decode
def test_overlaps(m3d, golden):
    g = golden("overlaps")
    assert np.array_equal(m3d.bbox_overlaps3d(dev(g["boxes"]), dev(g["query"])).cpu().numpy(), g["out"])
    rs = np.random.RandomState(1)
    a = rs.uniform(0, 50, (300, 6)).astype(np.float32); a[:, 3:] += a[:, :3]
    q = rs.uniform(0, 50, (77, 6)).astype(np.float32); q[:, 3:] += q[:, :3]
    assert np.array_equal(m3d.bbox_overlaps3d(dev(a), dev(q)).cpu().numpy(), O.bbox_overlaps_3d(a, q))


def test_bbox_transform(m3d, golden):
    g = golden("boxes")
    t1 = m3d.bbox_transform3d(dev(g["boxes"]), dev(g["d1"])).cpu().numpy()
    t2 = m3d.bbox_transform3d(dev(g["boxes"]), dev(g["d2"]), tuple(g["w2"])).cpu().numpy()
    # device exp() vs NumPy exp(): fp64 last-ulp differences can move the fp32 rounding -> 1 fp32 ulp
    for got, ref in ((t1, g["t1"]), (t2, g["t2"])):
        assert np.allclose(got, ref, rtol=2e-7, atol=1e-5)
        assert (got == ref).mean() > 0.98
    c2 = m3d.bbox_transform3d(dev(g["boxes"]), dev(g["d2"]), tuple(g["w2"]), clip_to=(64, 200, 200)).cpu().numpy()
    assert np.allclose(c2, g["c2"], rtol=2e-7, atol=1e-5)
    assert c2.min() >= 0 and c2[:, 0::6].max() <= 199 and c2[:, 2::6].max() <= 63


# ------------------------------------------------------------------ proposals
@pytest.mark.parametrize("tag,sizes,ratios", [
    ("n", (10, 27, 33, 38, 42, 46, 50), [[1.0, 0.5], [0.5, 0.5], [2., 0.5], [0.2, 0.5], [3., 2.]]),
    ("s", (10, 12, 14, 16, 18, 20, 22, 24, 28, 30, 34, 36, 38, 40), [[1.0, 1.0]])])
def test_generate_proposals_golden(m3d, golden, tag, sizes, ratios):
    g = golden("proposals")
    stride = float(g[tag + "_stride"])
    anchors = O.generate_anchors_3d(stride, sizes, ratios)
    rois, probs, kidx = m3d.generate_proposals3d(dev(g[tag + "_scores"][0]), dev(g[tag + "_deltas"][0]), anchors, stride,
                                                 g[tag + "_im_info"][0], int(g["pre"]), int(g["post"]), float(g[tag + "_thr"]))
    assert np.array_equal(kidx.cpu().numpy(), g[tag + "_keep_idx"])
    assert np.array_equal(probs.cpu().numpy(), g[tag + "_probs"])
    assert np.allclose(rois.cpu().numpy(), g[tag + "_rois"], rtol=2e-7, atol=1e-5)


def test_generate_proposals_vs_oracle_full_size_with_ties(m3d):
    rs = np.random.RandomState(3)
    A, S, H, W = 35, 16, 16, 16                         # config[1]/[2] size: 143 360 anchors
    cfg = O.Cfg()
    sc = rs.uniform(0, 1, (A, S, H, W)).astype(np.float32)
    sc[rs.uniform(0, 1, sc.shape) > 0.995] = 1.0        # saturated sigmoid: exact ties at the top
    dl = (rs.randn(6 * A, S, H, W) * 0.2).astype(np.float32)
    info = np.array([128., 128., 128., 1.0])
    r0, p0, k0 = O.generate_proposals_3d(sc, dl, info, cfg.anchors, 8, 1000, 1000, 0.15, 0)
    r1, p1, k1 = m3d.generate_proposals3d(dev(sc), dev(dl), cfg.anchors, 8., info, 1000, 1000, 0.15)
    assert np.array_equal(k1.cpu().numpy(), k0)
    assert np.array_equal(p1.cpu().numpy(), p0)
    assert np.allclose(r1.cpu().numpy(), r0, rtol=2e-7, atol=1e-5)
    # properties: scores sorted descending, boxes inside the image
    p = p1.cpu().numpy().ravel()
    assert np.all(p[:-1] >= p[1:])
    r = r1.cpu().numpy()
    assert r[:, 1:].min() >= 0 and r[:, 1:].max() <= 127


# ------------------------------------------------------------------ RoIAlign3D
def roi_forward_within_its_bound(f, rois, res, scale, ratio, got):
    """the per-element bound of the fp32 forward (tests/roi_align_forward_cases.py) on top of a test's own tolerance"""
    import roi_align_forward_cases as Fc
    v = Fc.compare(got, Fc.reference(f, rois, f.shape, (res, res, res), scale, ratio))
    assert v.outside == 0 and v.nonzero == 0, Fc.describe(v)


@pytest.mark.parametrize("shape,R,res,ratio", [((1, 8, 8, 8, 8), 5, 7, 2), ((2, 16, 6, 9, 11), 33, 7, 2),
                                                ((1, 4, 5, 6, 7), 9, 3, 0), ((1, 256, 16, 16, 16), 200, 7, 2)])
def test_roi_align_forward_bit_exact(m3d, shape, R, res, ratio):
    rs = np.random.RandomState(R)
    f = rs.randn(*shape).astype(np.float32)
    B, _, S, H, W = shape
    c = rs.uniform(-8, 8 * max(S, H, W) + 8, (R, 3)); s = rs.uniform(1, 60, (R, 3))
    rois = np.hstack((rs.randint(0, B, (R, 1)), c - s / 2, c + s / 2)).astype(np.float32)
    rois[0, 4:] = rois[0, 1:4] - 3          # malformed (x2 < x1)
    rois[1, 1:] = 4000.                     # fully outside
    got = m3d.roi_align3d_forward(dev(f), dev(rois), res, res, res, 0.125, ratio, exact=True).cpu().numpy()
    ref = O.roi_align_3d_forward(f, rois, res, res, res, 0.125, ratio)
    assert got.shape == ref.shape and np.array_equal(got, ref)          # reference operation order: bit-exact
    fast = m3d.roi_align3d_forward(dev(f), dev(rois), res, res, res, 0.125, ratio).cpu().numpy()
    assert np.abs(fast - ref).max() <= 1e-5 * np.abs(f).max()            # separable form: tolerance 1e-5 * max|f|
    assert np.array_equal(fast == 0, ref == 0) or np.abs(fast[ref == 0]).max() < 1e-6
    if R * shape[1] <= 1024:                 # the fp64 reference is cheap here
        roi_forward_within_its_bound(f, rois, res, 0.125, ratio, fast)


@pytest.mark.parametrize("B,C,dims,R", [(4, 256, (16, 16, 16), 400), (1, 128, (16, 40, 40), 300), (2, 64, (8, 25, 25), 150), (1, 96, (12, 14, 16), 80)])
def test_roi_align_matrix_core_form_for_small_sub_volumes(m3d, B, C, dims, R):
    """Round 6: with the feature maps' largest magnitude, RoIs whose sub-volume has <= 128 voxels run as ONE GEMM per RoI on the f16 matrix
    cores (out[c][bin] = sum_k f[c][k] M[k][bin], f16x2 split: csrc/roi_align3d.hip roi_align3d_fwd_gemm_kernel); the others through the
    separable kernels.  Against the oracle (reference operation order) within the fast mode's 1e-5 max |f|, against the separable form
    within 2e-6 max |f|; RoIs of every class in one call (tiny, <= 64, <= 128, larger, wide-bin, malformed, outside), channel counts
    that give a wave two, one or no channel block; a loose bound; no NaN marker left behind."""
    rs = np.random.RandomState(C + R)
    S, H, W = dims
    f = (rs.randn(B, C, S, H, W) * np.exp(rs.randn(B, C, 1, 1, 1))).astype(np.float32)
    ext = 8.0 * np.array([W, H, S])
    c = rs.uniform(0, 1, (R, 3)) * ext
    kind = rs.randint(0, 5, (R, 1))
    s = np.where(kind == 0, rs.uniform(2, 16, (R, 3)), np.where(kind == 1, rs.uniform(12, 30, (R, 3)), np.where(kind == 2, rs.uniform(20, 45, (R, 3)),
        np.where(kind == 3, rs.uniform(40, 90, (R, 3)), rs.uniform(200, 400, (R, 3))))))
    rois = np.hstack((rs.randint(0, B, (R, 1)), c - s / 2, c + s / 2)).astype(np.float32)
    rois[0, 4:] = rois[0, 1:4] - 3          # malformed (x2 < x1)
    rois[1, 1:] = 4000.                     # fully outside
    rois[2, 1:] = [-30, -30, -30, 6, 6, 6]  # mostly outside: samples below -1 contribute 0
    fd, rd = dev(f), dev(rois)
    ref = O.roi_align_3d_forward(f, rois, 7, 7, 7, 0.125, 2)
    sep = m3d.roi_align3d_forward(fd, rd, 7, 7, 7, 0.125, 2).cpu().numpy()
    fmax = np.abs(f).max()
    for bound in (m3d.ops.absmax(fd), m3d.ops.absmax(fd) * 64.0):
        got = m3d.roi_align3d_forward(fd, rd, 7, 7, 7, 0.125, 2, feat_absmax=bound).cpu().numpy()
        assert not np.isnan(got).any()
        assert np.abs(got - ref).max() <= 1e-5 * fmax
        assert np.abs(got - sep).max() <= 2e-6 * fmax, np.abs(got - sep).max() / fmax
        assert np.abs(got[ref == 0]).max() <= 1e-6 * fmax
    # per batch item the error is relative to the whole tensor's largest value (one scale for the operand): a quiet item next to a loud one
    # keeps 22 bits down to 2^-18 of the largest - checked on the item with the smallest values
    q = int(np.argmin([np.abs(f[b]).max() for b in range(B)]))
    sel = rois[:, 0] == q
    if sel.sum() > 3:
        assert np.abs(got[sel] - ref[sel]).max() <= 1e-5 * fmax
    # some RoIs must really have gone each way (the marker classes are the kernel's business; here: sub-volume sizes on both sides of 128)
    from_small = (s.max(1) < 30).sum(); from_large = (s.min(1) > 45).sum()
    assert from_small > 5 and from_large > 5


@pytest.mark.parametrize("C", [64, 96, 40])
def test_roi_align_fast_and_complement_kernels_share_the_rois(m3d, C):
    """ratio 2, 7^3 bins: RoIs with bins wider than 4 voxels are declined by the fast kernel and done by the complement pass
    (C % 32 == 0 with 8-aligned chunks: the hand-over goes through a marker in the output; otherwise through the predicate)."""
    rs = np.random.RandomState(C)
    f = rs.randn(1, C, 12, 14, 16).astype(np.float32)
    R = 60
    c = rs.uniform(0, 120, (R, 3)); s = np.where(rs.uniform(0, 1, (R, 1)) < 0.4, rs.uniform(240, 420, (R, 3)), rs.uniform(4, 60, (R, 3)))
    rois = np.hstack((np.zeros((R, 1)), c - s / 2, c + s / 2)).astype(np.float32)
    ref = O.roi_align_3d_forward(f, rois, 7, 7, 7, 0.125, 2)
    fast = m3d.roi_align3d_forward(dev(f), dev(rois), 7, 7, 7, 0.125, 2).cpu().numpy()
    assert not np.isnan(fast).any()
    assert np.abs(fast - ref).max() <= 1e-5 * np.abs(f).max()
    roi_forward_within_its_bound(f, rois, 7, 0.125, 2, fast)
    # the heavy-first launch order (m3d_roi_align3d_forward_ws: RoIs taken by descending work) changes WHICH workgroup computes a row,
    # nothing of the row: bit-identical with the index-order launch, duplicated RoIs (equal cost: ties by index) included
    rois2 = np.vstack((rois, rois[:7], rois[::-1][:5])).astype(np.float32)
    a_ = m3d.roi_align3d_forward(dev(f), dev(rois2), 7, 7, 7, 0.125, 2, ordered=True)
    b_ = m3d.roi_align3d_forward(dev(f), dev(rois2), 7, 7, 7, 0.125, 2, ordered=False)
    assert torch.equal(a_, b_) and torch.equal(a_[:R].cpu(), torch.from_numpy(fast))


def test_roi_align_bad_cols_and_empty(m3d):
    f = torch.zeros((1, 2, 4, 4, 4), device="cuda")
    with pytest.raises(m3d.M3DError):
        m3d.roi_align3d_forward(f, torch.zeros((3, 5), device="cuda"), 7, 7, 7, 0.125, 2)   # roi_align_cuda_3d.c:19-22
    assert m3d.roi_align3d_forward(f, torch.zeros((0, 7), device="cuda"), 7, 7, 7, 0.125, 2).shape == (0, 2, 7, 7, 7)


def test_roi_align_backward(m3d):
    rs = np.random.RandomState(9)
    shape = (2, 6, 5, 7, 8)
    rois = np.array([[1, 4, 4, 4, 40, 36, 30], [0, 0, 0, 0, 20, 20, 20], [0, -20, 3, 5, 70, 44, 39]], np.float32)
    top = rs.rand(3, 6, 3, 3, 3).astype(np.float32)
    got = m3d.roi_align3d_backward(dev(top), dev(rois), shape, 3, 3, 3, 0.125, 2).cpu().numpy()
    ref = O.roi_align_3d_backward(top, rois, shape, 3, 3, 3, 0.125, 2)
    assert np.allclose(got, ref, rtol=1e-5, atol=1e-6)      # float atomics: order differs (as in the reference)


# ------------------------------------------------------------------ conv / pool
def _conv_case(m3d, B, cin, cout, D, H, W, k, seed, **kw):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cin, D, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, k, generator=g) * (2.0 / (cin * k ** 3)) ** 0.5
    conv = m3d.PackedConv3d(w.cuda())
    y = conv(x.cuda(), **kw).cpu()
    ref = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, k // 2)
    return y, ref


@pytest.mark.parametrize("B,cin,cout,D,H,W,k", [
    (1, 1, 32, 8, 16, 40, 5), (1, 32, 64, 8, 12, 32, 3), (1, 64, 64, 9, 13, 33, 3), (2, 64, 128, 8, 8, 32, 3),
    (1, 128, 128, 6, 16, 16, 3), (1, 128, 256, 4, 8, 16, 3), (1, 256, 256, 5, 6, 7, 3), (1, 256, 245, 4, 16, 16, 1),
    (1, 128, 98, 3, 10, 40, 1), (1, 3, 5, 4, 5, 6, 3), (1, 1, 20, 6, 7, 9, 5), (1, 256, 256, 2, 25, 25, 3),
    (1, 128, 64, 16, 32, 32, 3), (1, 64, 32, 8, 32, 64, 3)])
def test_conv3d_forward_vs_fp64(m3d, B, cin, cout, D, H, W, k):
    y, ref = _conv_case(m3d, B, cin, cout, D, H, W, k, seed=cin * 7 + k)
    err = (y.double() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-4, err                                  # north_star: fp32 convs within 1e-4 relative
    assert err < 5e-6                                       # exact-fp32 MFMA: expect ~1e-6


def test_conv3d_matches_oracle_direct_and_epilogue(m3d):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 6, 5, 9, 34, generator=g)
    w = torch.randn(40, 6, 3, 3, 3, generator=g) * 0.1
    sc = torch.rand(40, generator=g) + 0.5
    sh = torch.randn(40, generator=g)
    off = torch.tensor([x.min().item()])
    ref = torch.from_numpy(O.conv3d_direct(x.numpy(), w.numpy(), None, in_offset=float(off), relu_w=True))
    ref = torch.relu(ref * sc.view(1, -1, 1, 1, 1) + sh.view(1, -1, 1, 1, 1))
    conv = m3d.PackedConv3d(w.cuda(), mode=m3d.W_RELU)
    y = conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True, in_offset=off.cuda()).cpu()
    assert (y - ref).abs().max().item() / ref.abs().max().item() < 1e-5


def test_conv3d_dgrad_pack(m3d):
    g = torch.Generator().manual_seed(6)
    w = torch.randn(48, 20, 3, 3, 3, generator=g) * 0.1
    gy = torch.randn(1, 48, 6, 10, 32, generator=g)
    ref = torch.nn.grad.conv3d_input((1, 20, 6, 10, 32), w.double(), gy.double(), 1, 1)
    dg = m3d.PackedConv3d(w.cuda(), mode=m3d.W_DGRAD)
    y = dg(gy.cuda()).cpu()
    assert (y.double() - ref).abs().max().item() / ref.abs().max().item() < 5e-6


@pytest.mark.parametrize("B,cin,cout,D,H,W,k", [
    (2, 5, 7, 5, 6, 19, 3), (1, 40, 70, 8, 9, 17, 3), (1, 64, 64, 16, 16, 32, 3), (1, 64, 33, 6, 8, 16, 1),
    (1, 256, 245, 4, 8, 8, 1), (2, 1, 32, 9, 10, 21, 5), (1, 1, 20, 6, 7, 40, 5), (1, 128, 128, 4, 4, 16, 3)])
def test_conv3d_wgrad_and_bias_grad_vs_fp64(m3d, B, cin, cout, D, H, W, k):
    """dW / db of the stride-1 same conv (MFMA split-K wgrad, deterministic reduction) against torch's fp64 autograd."""
    g = torch.Generator().manual_seed(B + cin + cout + k)
    x = torch.randn(B, cin, D, H, W, generator=g)
    gy = torch.randn(B, cout, D, H, W, generator=g)
    ref = torch.nn.grad.conv3d_weight(x.double(), (cout, cin, k, k, k), gy.double(), 1, k // 2)
    dw = m3d.conv3d_wgrad(x.cuda(), gy.cuda(), k)
    dw2 = m3d.conv3d_wgrad(x.cuda(), gy.cuda(), k)
    assert torch.equal(dw, dw2)                              # fixed-order split-K reduction
    err = (dw.cpu().double() - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-4, err
    assert err < 1e-5, err
    db = m3d.conv3d_bias_grad(gy.cuda()).cpu().double()
    rb = gy.double().sum((0, 2, 3, 4))
    assert (db - rb).abs().max().item() / rb.abs().max().item() < 1e-5


@pytest.mark.parametrize("B,cin,cout,D,H,W", [
    (1, 32, 64, 6, 9, 64), (1, 64, 64, 5, 8, 70), (2, 5, 7, 4, 5, 48), (1, 64, 128, 6, 11, 32), (1, 128, 128, 4, 6, 37),
    (1, 33, 40, 3, 4, 24), (1, 16, 96, 7, 13, 129), (1, 256, 256, 3, 25, 25), (1, 2, 200, 2, 3, 100)])
@pytest.mark.parametrize("two_d", [False, True])
def test_conv3d_winograd_vs_fp64(m3d, B, cin, cout, D, H, W, two_d):
    """The F(2,3)-along-x and F(2x2,3x3)-on-(y,x) kernels compute the same conv + scale/shift + ReLU (+ fused pool) as
    the direct kernel (every tile configuration, ragged sizes, odd widths / heights -> unpaired stores)."""
    g = torch.Generator().manual_seed(B * 1000 + cin + cout + W)
    x = torch.randn(B, cin, D, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    ref = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 1)
    conv = m3d.WinoConv3d(w.cuda(), two_d=two_d)
    y = conv(x.cuda()).cpu().double()
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-4, err                                   # north_star tolerance
    # what the fp32 transforms actually deliver: F(2,3) along x a few 1e-7; the default 2-D family, F(2x4,3x3) (interpolation points
    # 0, +-1, +-2, inf along x: coefficients up to 8), about twice F(2x2,3x3)'s error - 5.6e-6 measured at 256 input channels
    tight = 2e-5 if two_d else 5e-6
    assert err < tight, err
    ref2 = torch.relu(ref * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    y2 = conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True).cpu().double()
    assert (y2 - ref2).abs().max().item() / ref2.abs().max().item() < tight
    if conv.supports_pool(W) and D >= 2 and H >= 2:           # 2-D kernel: 64- and 32-wide tiles have the fused pool (W >= 24)
        yp = conv.pooled(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True).cpu().double()
        refp = torch.nn.functional.max_pool3d(ref2, 2, 2)
        assert yp.shape == refp.shape
        assert (yp - refp).abs().max().item() / refp.abs().max().item() < tight


def test_conv3d_winograd_local_family_is_exactly_local(m3d):
    """WinoConv3d(local=True) = the F(2x2,3x3) family: an output depends on nothing outside its own 3 x 3 (y, x) support, not even by
    rounding, so a block of zeros next to a block of huge values stays EXACTLY zero (what the PRM strip layout relies on: windows of
    different peaks are one zero column apart).  The default family's F(4,3) along x is local only up to ~1e-7 of the neighbour."""
    g = torch.Generator().manual_seed(9)
    cin, cout, D, H, W = 64, 64, 4, 16, 128
    x = torch.zeros(1, cin, D, H, W)
    x[..., 66:] = torch.rand(1, cin, D, H, W - 66, generator=g) * 1e6          # columns 0..64 zero, column 65 the gap, 66.. huge
    w = torch.rand(cout, cin, 3, 3, 3, generator=g)
    ref = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 1)
    local = m3d.WinoConv3d(w.cuda(), two_d=True, local=True)(x.cuda()).cpu()
    assert float(local[..., :65].abs().max()) == 0.0                            # outputs whose support is all zeros: exactly zero
    assert (local.double() - ref).abs().max().item() / ref.abs().max().item() < 5e-6
    dflt = m3d.WinoConv3d(w.cuda(), two_d=True)(x.cuda()).cpu()
    assert (dflt.double() - ref).abs().max().item() / ref.abs().max().item() < 2e-5
    assert float(dflt[..., :62].abs().max()) == 0.0                             # beyond F(4,3)'s 6-wide footprint nothing arrives either


@pytest.mark.parametrize("n", [16, 18, 38, 40])
def test_quad_aligned_strip_keeps_peaks_apart_under_the_f24_family(m3d, n):
    """The PRM strip layout for the F(2x4,3x3) family (m3d_prm_strip_geometry mode 2): every window starts on the same residue
    mod 4 and no output quad that holds a window's columns reads another window's columns.  So a window's outputs must be IDENTICAL BIT
    FOR BIT whether its neighbours hold zeros or values a million times larger - F(4,3)'s rounding-level 6-wide footprint never leaves
    the window and its zero gap."""
    P, cin, cout = 5, 16, 32
    pitch, lead, L = m3d.strip_geometry(n, 2, P)
    assert pitch % 4 == 0 and pitch > n and 0 <= lead < 4 and L == P * pitch + (4 if lead else 0)
    p1, l1, L1 = m3d.strip_geometry(n, 1, P)
    assert (p1, l1, L1) == (n + 1, 0, P * (n + 1))
    g = torch.Generator().manual_seed(n)
    w = torch.rand(cout, cin, 3, 3, 3, generator=g) - 0.3
    conv = m3d.WinoConv3d(w.cuda(), two_d=True)                          # the library's default family: F(2x4,3x3)
    wins = [torch.randn(cin, 6, n, n, generator=g) * (1e6 if k % 2 else 1.0) for k in range(P)]
    full = torch.zeros(1, cin, 6, n, L)
    for k in range(P):
        full[0, ..., lead + k * pitch:lead + k * pitch + n] = wins[k]
    yf = conv(full.cuda()).cpu()
    for k in range(P):
        alone = torch.zeros_like(full)
        alone[0, ..., lead + k * pitch:lead + k * pitch + n] = wins[k]
        ya = conv(alone.cuda()).cpu()
        sl = slice(lead + k * pitch, lead + k * pitch + n)
        assert torch.equal(yf[..., sl], ya[..., sl]), (n, k)
        ref = torch.nn.functional.conv3d(wins[k][None].double(), w.double(), None, 1, 1)
        assert (ya[..., sl].double() - ref).abs().max().item() / ref.abs().max().item() < 2e-5


@pytest.mark.parametrize("B,cin,cout,D,H,W", [(1, 64, 64, 6, 8, 64), (2, 32, 40, 4, 10, 70), (1, 128, 128, 4, 6, 32), (1, 16, 33, 5, 7, 50)])
def test_conv3d_winograd_2d_pool_argmax(m3d, B, cin, cout, D, H, W):
    """F(2x2,3x3) + BN + ReLU + MaxPool3d(2,2) + argmax in one launch == the same kernel's un-pooled output pushed through
    m3d_maxpool3d_2x_forward (values bit for bit, indices with the first-maximum rule; ReLU zeros make ties common)."""
    g = torch.Generator().manual_seed(cin + cout + W)
    x = torch.randn(B, cin, D, H, W, generator=g).cuda()
    w = (torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5).cuda()
    sc = (torch.rand(cout, generator=g) + 0.5).cuda()
    sh = torch.randn(cout, generator=g).cuda()
    conv = m3d.WinoConv3d(w, two_d=True)
    y = conv(x, scale=sc, shift=sh, relu=True)                # may come from another tile configuration: equal to a few ulp
    ref = torch.nn.functional.max_pool3d(y, 2, 2)
    out, am = conv.pooled(x, scale=sc, shift=sh, relu=True, return_argmax=True)
    tol = 1e-5 * float(ref.abs().max())
    assert out.shape == ref.shape and am.shape == ref.shape and am.dtype == torch.uint8 and int(am.max()) <= 7
    assert (out - ref).abs().max().item() <= tol
    assert torch.equal(conv.pooled(x, scale=sc, shift=sh, relu=True), out)              # same kernel without the index output
    # the index points at a child that holds the maximum ...
    PD, PH, PW = ref.shape[-3:]
    yc = y[..., :2 * PD, :2 * PH, :2 * PW].reshape(B, cout, PD, 2, PH, 2, PW, 2).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(B, cout, PD, PH, PW, 8)
    picked = torch.gather(yc, 5, am.long().unsqueeze(-1)).squeeze(-1)
    assert (picked - out).abs().max().item() <= tol
    # ... and at the FIRST one in (dz, dy, dx) order where they tie exactly (all eight children cut to 0 by the ReLU)
    allzero = (yc == 0).all(-1) & (out == 0)
    assert int(allzero.sum()) > 0 and int(am[allzero].max()) == 0


@pytest.mark.parametrize("B,cin,cout,D,H,W", [
    (1, 32, 64, 6, 8, 64), (2, 64, 64, 4, 12, 32), (1, 16, 96, 7, 13, 129), (1, 64, 128, 6, 11, 37), (1, 128, 128, 4, 6, 24),
    (1, 256, 256, 4, 16, 16), (1, 128, 40, 3, 9, 17), (1, 48, 70, 2, 4, 12), (1, 256, 245, 8, 25, 23)])
def test_conv3d_f16x2_z_winograd_vs_fp64(m3d, B, cin, cout, D, H, W):
    """csrc/conv3d_zw.hip (f16x2 split, F(2,3) along z): conv + scale/shift + ReLU (+ fused pool) against torch's fp64 conv, both column-block
    widths, ragged tiles, odd depths, channel counts that are not multiples of 64; the output bound the epilogue leaves for the next layer."""
    g = torch.Generator().manual_seed(B * 1000 + cin + cout + W)
    x = torch.relu(torch.randn(B, cin, D, H, W, generator=g)) * 3.0          # activations as the layers see them: >= 0
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    ref = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 1)
    conv = m3d.ZwConv3d(w.cuda())
    assert conv.supports((D, H, W))
    xm = m3d.ZwConv3d.bound_of(x.cuda())
    assert float(xm[0]) == float(x.abs().max()) and float(xm[1:].abs().max()) == 0.0
    y, ym = conv(x.cuda(), xm)
    y = y.cpu().double()
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-4, err                                   # north_star tolerance
    assert err < 3e-6, err                                   # what 22-bit operands and fp32 accumulation deliver
    assert abs(float(ym.max()) - float(y.abs().max())) == 0.0
    ref2 = torch.relu(ref * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    y2, ym2 = conv(x.cuda(), xm, scale=sc.cuda(), shift=sh.cuda(), relu=True)
    assert (y2.cpu().double() - ref2).abs().max().item() / ref2.abs().max().item() < 3e-6
    assert float(ym2.max()) == float(y2.max())
    # signed input (no ReLU in front), and a bound larger than the data (a producer's bound is allowed to be loose)
    xs = torch.randn(B, cin, D, H, W, generator=g)
    refs = torch.nn.functional.conv3d(xs.double(), w.double(), None, 1, 1)
    loose = m3d.ZwConv3d.bound_of(xs.cuda()) * 7.0
    ys, _ = conv(xs.cuda(), loose)
    assert (ys.cpu().double() - refs).abs().max().item() / refs.abs().max().item() < 3e-6
    if conv.supports((D, H, W), pool=True):
        yp, ymp = conv(x.cuda(), xm, scale=sc.cuda(), shift=sh.cuda(), relu=True, pool=True)
        refp = torch.nn.functional.max_pool3d(ref2, 2, 2)
        assert yp.shape == refp.shape
        assert (yp.cpu().double() - refp).abs().max().item() / refp.abs().max().item() < 3e-6
        assert float(ymp.max()) == float(yp.max())
        assert torch.equal(yp, torch.nn.functional.max_pool3d(y2, 2, 2))        # the fused pool is the un-pooled kernel's output, pooled


def test_conv3d_f16x2_operand_bound_is_tied_to_the_tensor_version(m3d):
    """The bound a producing launch leaves on its output tensor (`_m3d_bound`) is only used while the tensor is unchanged: after an in-place
    write the model sweeps the tensor again (a stale bound would overflow fp16 silently)."""
    from m3d.model import DetectorM3D
    g = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(1, 16, 4, 8, 32, generator=g)).cuda()
    w = (torch.randn(32, 16, 3, 3, 3, generator=g) * 0.05).cuda()
    conv = m3d.ZwConv3d(w)
    y, ym = conv(x, m3d.ZwConv3d.bound_of(x), relu=True)
    y._m3d_bound = (ym, y._version)
    assert DetectorM3D._bound(y) is ym
    y.mul_(1000.0)                                           # in place: the recorded bound is 1000 x too small now
    b2 = DetectorM3D._bound(y)
    assert b2 is not ym and float(b2.max()) == float(y.abs().max())
    w2 = (torch.randn(16, 32, 3, 3, 3, generator=g) * 0.05).cuda()
    z, _ = m3d.ZwConv3d(w2)(y, b2)
    ref = torch.nn.functional.conv3d(y.cpu().double(), w2.cpu().double(), padding=1)
    assert (z.cpu().double() - ref).abs().max().item() / ref.abs().max().item() < 3e-6


@pytest.mark.parametrize("B,cin,cout,D,H,W", [(1, 128, 256, 16, 16, 16), (1, 256, 256, 8, 25, 23), (2, 20, 40, 3, 13, 12),
                                                (1, 256, 70, 5, 9, 17), (1, 6, 33, 2, 30, 21)])
def test_conv3d_winograd_2d_split_k_small_maps(m3d, B, cin, cout, D, H, W):
    """Maps 12..23 wide (the 16^3 stage-4 layers): 16x16x2 tiles, K split over workgroups, fixed-order reduction."""
    g = torch.Generator().manual_seed(cin + cout + W)
    x = torch.randn(B, cin, D, H, W, generator=g)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    ref = torch.relu(torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 1) * sc.double().view(1, -1, 1, 1, 1)
                     + sh.double().view(1, -1, 1, 1, 1))
    conv = m3d.WinoConv3d(w.cuda(), two_d=True)
    assert conv.supports(W)
    y = conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True)
    assert torch.equal(y, conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True))      # deterministic
    assert (y.cpu().double() - ref).abs().max().item() / ref.abs().max().item() < 2e-5       # F(2x4,3x3): see test_conv3d_winograd_vs_fp64


@pytest.mark.parametrize("B,cout,D,H,W", [(1, 32, 6, 8, 64), (2, 32, 5, 7, 70), (1, 20, 4, 6, 33), (1, 48, 3, 5, 128), (1, 32, 9, 3, 37)])
def test_conv3d_stem_winograd_vs_fp64(m3d, B, cout, D, H, W):
    """conv1a through the F(2,5)-along-x kernel (+ fused pool): same result as the direct stem kernel to fp32 rounding;
    ragged sizes, the head / tail quads of the tensor, more than one 32-channel block."""
    g = torch.Generator().manual_seed(cout + W)
    x = torch.randn(B, 1, D, H, W, generator=g)
    w = torch.randn(cout, 1, 5, 5, 5, generator=g) * (2.0 / 125) ** 0.5
    sc = torch.rand(cout, generator=g) + 0.5
    sh = torch.randn(cout, generator=g)
    ref = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 2)
    conv = m3d.StemWinoConv3d(w.cuda())
    y = conv(x.cuda()).cpu().double()
    err = (y - ref).abs().max().item() / ref.abs().max().item()
    assert err < 1e-4, err
    assert err < 1e-5, err
    ref2 = torch.relu(ref * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    y2 = conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True).cpu().double()
    assert (y2 - ref2).abs().max().item() / ref2.abs().max().item() < 1e-5
    if D >= 2 and H >= 2:
        yp = conv.pooled(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True).cpu().double()
        refp = torch.nn.functional.max_pool3d(ref2, 2, 2)
        assert yp.shape == refp.shape and (yp - refp).abs().max().item() / refp.abs().max().item() < 1e-5


@pytest.mark.parametrize("tune", [4, 8])
def test_conv3d_stem_winograd_kernels_agree(m3d, tune):
    """The two stem kernels (rows kernel with 4 / 8 planes per workgroup - the library picks by size) on a
    ragged volume deeper than one tile, odd D / H, W not a multiple of the tile, 40 channels (a partial block of 8): each against fp64,
    and the pooled result bit-identical to max_pool3d of the kernel's own unpooled result."""
    from m3d import _lib
    g = torch.Generator().manual_seed(tune)
    x = torch.randn(2, 1, 19, 21, 75, generator=g)
    w = torch.randn(40, 1, 5, 5, 5, generator=g) * (2.0 / 125) ** 0.5
    sc = torch.rand(40, generator=g) - 0.3          # some negative scales: the maximum is taken after the scale
    sh = torch.randn(40, generator=g)
    ref = torch.relu(torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 2) * sc.double().view(1, -1, 1, 1, 1)
                     + sh.double().view(1, -1, 1, 1, 1))
    with _lib.tuning():                              # the knob lives in libm3d_tune.so only; the release library has no mutable state
        _lib.set_option("tune_stem", tune)
        conv = m3d.StemWinoConv3d(w.cuda())
        y = conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True)
        yp = conv.pooled(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True)
    assert (y.cpu().double() - ref).abs().max().item() / ref.abs().max().item() < 1e-5
    assert torch.equal(yp, torch.nn.functional.max_pool3d(y, 2, 2))


@pytest.mark.parametrize("fam", [2, 4])
def test_conv3d_winograd_ab_families_agree_with_fp64(m3d, fam):
    """The two kernel families behind option tune_wino2 (299: F(2x2) eta-split, 499: F(2x4), the default, named explicitly)
    stay correct: plain and pooled forward of a 64 -> 128 layer on a ragged 9 x 22 x 70 map against fp64."""
    from m3d import _lib
    g = torch.Generator().manual_seed(fam)
    x = torch.randn(2, 64, 9, 22, 70, generator=g)
    w = torch.randn(128, 64, 3, 3, 3, generator=g) * (2.0 / (64 * 27)) ** 0.5
    sc = torch.rand(128, generator=g) + 0.5
    sh = torch.randn(128, generator=g)
    ref = torch.relu(torch.nn.functional.conv3d(x.double(), w.double(), None, 1, 1) * sc.double().view(1, -1, 1, 1, 1)
                     + sh.double().view(1, -1, 1, 1, 1))
    with _lib.tuning():
        _lib.set_option("tune_wino2", fam * 100 + 99)
        conv = m3d.WinoConv3d(w.cuda(), two_d=True)
        y = conv(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True)
        yp = conv.pooled(x.cuda(), scale=sc.cuda(), shift=sh.cuda(), relu=True) if conv.supports_pool(70) else None
    assert (y.cpu().double() - ref).abs().max().item() / ref.abs().max().item() < 2e-5
    if yp is not None:
        assert torch.equal(yp, torch.nn.functional.max_pool3d(y, 2, 2))


def test_conv3d_winograd_rejects_narrow_maps(m3d):
    conv = m3d.WinoConv3d(torch.randn(8, 4, 3, 3, 3).cuda())
    assert not conv.supports(16) and conv.supports(24) and not conv.supports_pool(32)
    with pytest.raises(m3d.M3DError):
        conv(torch.randn(1, 4, 4, 16, 16).cuda())
    conv2 = m3d.WinoConv3d(torch.randn(8, 4, 3, 3, 3).cuda(), two_d=True)
    assert conv2.supports(16) and not conv2.supports(11)
    with pytest.raises(m3d.M3DError):
        conv2(torch.randn(1, 4, 4, 8, 8).cuda())


def test_conv3d_linearity_full_size(m3d):
    """Size-independent property at the BASELINE config[1] size (conv2b on 64^3): conv(a*x + y) = a*conv(x) + conv(y)."""
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(64, 64, 3, 3, 3, generator=g) * 0.03).cuda()
    conv = m3d.PackedConv3d(w)
    x = torch.randn(1, 64, 64, 64, 64, generator=g).cuda()
    y = torch.randn(1, 64, 64, 64, 64, generator=g).cuda()
    lhs = conv(2.0 * x + y)
    rhs = 2.0 * conv(x) + conv(y)
    assert (lhs - rhs).abs().max().item() / rhs.abs().max().item() < 1e-5


def test_maxpool(m3d):
    x = torch.randn(2, 5, 9, 10, 13)
    ref, idx = torch.nn.functional.max_pool3d(x, 2, 2, return_indices=True)
    out, am = m3d.maxpool3d_2x(x.cuda(), return_argmax=True)
    assert torch.equal(out.cpu(), ref)
    go = torch.randn(ref.shape)
    gin = m3d.maxpool3d_2x_backward(go.cuda(), am, x.shape).cpu()
    xr = x.clone().requires_grad_()
    torch.nn.functional.max_pool3d(xr, 2, 2).backward(go)
    assert torch.equal(gin, xr.grad)
    assert m3d.reduce_min(x.cuda()).item() == x.min().item()


# ------------------------------------------------------------------ Otsu 2D
def test_otsu_golden(m3d, golden):
    g = golden("otsu")
    imgs = [g["img%d" % i].ravel() for i in range(6)]
    prms = [g["prm%d" % i].ravel() for i in range(6)]
    offs = np.concatenate(([0], np.cumsum([a.size for a in imgs]))).astype(np.int64)
    mask, kb, status = m3d.otsu2d_batch(torch.from_numpy(np.concatenate(imgs)).cuda(), torch.from_numpy(np.concatenate(prms)).cuda(),
                                        dev(offs))
    mask, kb, status = mask.cpu().numpy(), kb.cpu().numpy(), status.cpu().numpy()
    for i in range(6):
        assert status[i] == 0
        assert tuple(kb[i]) == tuple(g["kb%d" % i]), i
        assert np.array_equal(mask[offs[i]:offs[i + 1]].reshape(g["mask%d" % i].shape), g["mask%d" % i]), i


def test_otsu_vs_oracle_random(m3d):
    rs = np.random.RandomState(4)
    imgs, prms = [], []
    for i in range(12):
        shp = tuple(rs.randint(6, 40, 3))
        zz, yy, xx = np.mgrid[0:shp[0], 0:shp[1], 0:shp[2]]
        r = np.sqrt((zz - shp[0] / 2) ** 2 + (yy - shp[1] / 2) ** 2 + (xx - shp[2] / 2) ** 2)
        img = (rs.uniform(300, 3000) * np.exp(-(r / rs.uniform(3, 12)) ** 2) + 100 + rs.randn(*shp) * 20).clip(0, 65535).astype(np.uint16)
        prm = (255 * np.exp(-(r / rs.uniform(3, 10)) ** 2) * rs.uniform(0.6, 1.0, shp)).astype(np.uint8)
        a, b = (O.normalize_soma if i % 2 == 0 else O.normalize_nuclei)(img, prm)
        imgs.append(a); prms.append(b)
    offs = np.concatenate(([0], np.cumsum([a.size for a in imgs]))).astype(np.int64)
    mask, kb, status = m3d.otsu2d_batch(torch.from_numpy(np.concatenate([a.ravel() for a in imgs])).cuda(),
                                        torch.from_numpy(np.concatenate([a.ravel() for a in prms])).cuda(), dev(offs), 8192)
    mask, kb = mask.cpu().numpy(), kb.cpu().numpy()
    for i in range(12):
        m, k, b = O.otsu_py_2d_fast(imgs[i], prms[i])
        assert (k, b) == tuple(kb[i]), i
        assert np.array_equal(mask[offs[i]:offs[i + 1]].reshape(m.shape), m), i


# ------------------------------------------------------------------ drivers
def test_im_detect_all_vs_oracle(m3d):
    """core/test.py:54-177 counterpart: tiles + offsets + cross-tile NMS.  E2E parity is a set match within
    tolerance (1e-6 conv noise may flip an NMS decision sitting on the threshold)."""
    from m3d.model import DetectorM3D
    from m3d.infer import im_detect_all
    from m3d import tiling
    cfg = O.Cfg(mlp_dim=64, score_thresh=0.3, pre_nms_topN=300, post_nms_topN=100)
    P = O.make_params(stride=8, num_anchors=35, mlp_dim=64, seed=21)
    det = DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg)
    rs = np.random.RandomState(0)
    im = (rs.rand(20, 48, 40) * 500 + 10).astype(np.uint16)
    patch, ov = (16, 32, 32), 8
    got = im_detect_all(det, im, patch=patch, overlap=ov)[1]
    vol = tiling.norm1(im, np.float32).astype(np.float32)
    sidx, hidx, widx = tiling.tile_grid(vol.shape, patch, ov)
    alld = []
    for _, s, h, w in tiling.enumerate_tiles(sidx, hidx, widx):
        r = O.detect_tile(P, cfg, torch.from_numpy(vol[s:s + 16, h:h + 32, w:w + 32].copy()[None, None]))
        alld.append(r["cls_boxes"][1] + np.array([w, h, s, w, h, s, 0], np.float32))
    alld = np.vstack(alld)
    ref = alld[O.nms_3d(alld, cfg.nms)]
    assert abs(len(got) - len(ref)) <= max(2, len(ref) // 20)
    matched = sum(np.abs(ref - g).max(1).min() < 1e-2 for g in got)
    assert matched >= 0.95 * len(got)


@pytest.mark.parametrize("cin,cout,k,D,H,W", [(1, 32, 5, 8, 12, 64), (1, 20, 5, 6, 10, 34), (64, 64, 3, 8, 8, 64), (32, 48, 3, 7, 9, 33)])
def test_conv3d_fused_pool_equals_conv_then_pool(m3d, cin, cout, k, D, H, W):
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(2, cin, D, H, W, generator=g).cuda()
    w = (torch.randn(cout, cin, k, k, k, generator=g) * 0.1).cuda()
    sc = (torch.rand(cout, generator=g) + 0.5).cuda()
    sh = torch.randn(cout, generator=g).cuda()
    conv = m3d.PackedConv3d(w)
    assert conv.supports_pool(W)
    y = conv(x, scale=sc, shift=sh, relu=True)
    ref, am_ref = m3d.maxpool3d_2x(y, return_argmax=True)
    out, am = conv.pooled(x, scale=sc, shift=sh, relu=True, return_argmax=True)
    # the un-fused launch may use another channel-chunk size (different fp32 summation order), so the two are not bitwise
    # equal; what IS checked: each is within fp32 summation noise of the fp64 result (cin*k^3 <= 1728 products, |y| ~ 1-10:
    # bound 4e-6 * max|y|), and every element where they differ differs by at most that noise - no structural mismatch.
    y64 = torch.nn.functional.conv3d(x.double(), w.double(), None, 1, k // 2) * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1)
    ref64 = torch.nn.functional.max_pool3d(torch.relu(y64), 2, 2)
    noise = 4e-6 * ref64.abs().max().item()
    assert (out.double() - ref64).abs().max().item() <= noise and (ref.double() - ref64).abs().max().item() <= noise
    assert (out - ref).abs().max().item() <= 2 * noise
    assert torch.allclose(out, ref, rtol=1e-5, atol=1e-5)
    tref, _ = torch.nn.functional.max_pool3d(y.cpu(), 2, 2, return_indices=True)
    assert torch.allclose(out.cpu(), tref, rtol=1e-5, atol=1e-5)
    # argmax consistency: the window element the index points at is the pooled maximum
    B, Cc, OD, OH, OW = out.shape
    q = am.long()
    zz = torch.arange(OD, device="cuda").view(1, 1, OD, 1, 1) * 2 + (q >> 2)
    yy = torch.arange(OH, device="cuda").view(1, 1, 1, OH, 1) * 2 + ((q >> 1) & 1)
    xx = torch.arange(OW, device="cuda").view(1, 1, 1, 1, OW) * 2 + (q & 1)
    picked = y[torch.arange(B, device="cuda").view(B, 1, 1, 1, 1), torch.arange(Cc, device="cuda").view(1, Cc, 1, 1, 1), zz, yy, xx]
    assert torch.allclose(picked, out, rtol=1e-5, atol=1e-5)
    assert (am == am_ref).float().mean() > 0.999
    differ = am != am_ref                              # argmax may differ only where two window elements tie to fp32 noise
    if differ.any():
        qr = am_ref.long()
        zr = torch.arange(OD, device="cuda").view(1, 1, OD, 1, 1) * 2 + (qr >> 2)
        yr = torch.arange(OH, device="cuda").view(1, 1, 1, OH, 1) * 2 + ((qr >> 1) & 1)
        xr = torch.arange(OW, device="cuda").view(1, 1, 1, 1, OW) * 2 + (qr & 1)
        picked_ref = y[torch.arange(B, device="cuda").view(B, 1, 1, 1, 1), torch.arange(Cc, device="cuda").view(1, Cc, 1, 1, 1), zr, yr, xr]
        assert (picked - picked_ref)[differ].abs().max().item() <= 2 * noise


# ------------------------------------------------------------------ PRM post-processing -> Otsu
@pytest.mark.parametrize("mode", ["soma", "nuclei"])
def test_quantize_normalize_otsu_chain_bit_exact(m3d, mode):
    """uint8 PRM quantisation (infer_simple.py:233-238) -> box crop + normalisation (binarization_*.py) ->
    otsu_py_2d_fast, all on device, against the NumPy restatements in the oracle (integer outputs: bit-exact)."""
    rs = np.random.RandomState(11)
    D, H, W = 20, 36, 40
    zz, yy, xx = np.mgrid[0:D, 0:H, 0:W]
    img = (rs.randn(D, H, W) * 12 + 110).clip(0, 65535)
    R = 5
    prms, boxes = [], []
    for r in range(R):
        c = np.array([rs.uniform(5, D - 5), rs.uniform(8, H - 8), rs.uniform(8, W - 8)])
        rad = rs.uniform(3, 6)
        d2 = (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2
        img += rs.uniform(300, 900) * np.exp(-d2 / (2 * rad * rad))
        p = np.exp(-d2 / (2 * (rad * 0.8) ** 2)).astype(np.float32) * (rs.rand(D, H, W).astype(np.float32) * 0.3 + 0.7)
        p[d2 > (3 * rad) ** 2] = 0
        prms.append(p / p.sum())
        h = int(2.2 * rad)
        lo = np.maximum(np.round(c).astype(int) - h, 0)
        hi = np.minimum(np.round(c).astype(int) + h, [D - 1, H - 1, W - 1])
        boxes.append([lo[2], lo[1], lo[0], hi[2], hi[1], hi[0]])
    img = img.clip(0, 65535).astype(np.uint16)
    prms = np.stack(prms).astype(np.float32)
    boxes = np.array(boxes, np.int32)
    q = m3d.prm_quantize_u8(dev(prms))
    q_ref = np.stack([O.quantize_prm_u8(p) for p in prms])
    assert np.array_equal(q.cpu().numpy(), q_ref)
    oi, op, offs = m3d.roi_normalize(torch.from_numpy(img).cuda(), q, dev(boxes), mode)
    mask, kb, status = m3d.otsu2d_batch(oi, op, offs, 4096)
    oi, op, offs, mask, kb = oi.cpu().numpy(), op.cpu().numpy(), offs.cpu().numpy(), mask.cpu().numpy(), kb.cpu().numpy()
    norm = O.normalize_soma if mode == "soma" else O.normalize_nuclei
    for r in range(R):
        x1, y1, z1, x2, y2, z2 = boxes[r]
        bi = img[z1:z2 + 1, y1:y2 + 1, x1:x2 + 1]
        bp = q_ref[r][z1:z2 + 1, y1:y2 + 1, x1:x2 + 1]
        a, b = norm(bi.copy(), bp.copy())
        assert np.array_equal(oi[offs[r]:offs[r + 1]].reshape(a.shape), a), r
        assert np.array_equal(op[offs[r]:offs[r + 1]].reshape(b.shape), b), r
        m, k, bb = O.otsu_py_2d_fast(a, b)
        assert (k, bb) == tuple(kb[r]) and np.array_equal(mask[offs[r]:offs[r + 1]].reshape(m.shape), m), r


# ------------------------------------------------------------------ reference fixtures straight into the device path
def test_box_results_golden_through_the_gpu_path(m3d, golden):
    """tests/golden/box_results.npz (the reference's own box_results_with_nms_and_limit, core/test.py:806-883) fed into
    DetectorM3D.box_results_with_nms_and_limit: identical kept scores / boxes / anchor indices, bit for bit."""
    from m3d.model import DetectorM3D
    g = golden("box_results")
    cfg = O.Cfg(mlp_dim=32)
    P = O.make_params(stride=8, num_anchors=35, mlp_dim=32, seed=0)
    det = DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg)
    sc, bx, cls_boxes, cls_keep = det.box_results_with_nms_and_limit(dev(g["scores"]), dev(g["boxes"]), dev(g["keep_idx"]))
    assert np.array_equal(sc.cpu().numpy(), g["o_scores"]) and np.array_equal(bx.cpu().numpy(), g["o_boxes"])
    assert np.array_equal(cls_boxes[1].cpu().numpy(), g["o_cls1"]) and np.array_equal(cls_keep[1].cpu().numpy(), g["o_keep1"])
    sc, bx, _, _ = det.box_results_with_nms_and_limit(dev(g["scores"]), dev(g["boxes"]))
    assert np.array_equal(sc.cpu().numpy(), g["p_scores"]) and np.array_equal(bx.cpu().numpy(), g["p_boxes"])
    det.cfg = O.Cfg(mlp_dim=32, detections_per_im=40)                 # cap semantics (:869-878)
    sc, _, _, ck = det.box_results_with_nms_and_limit(dev(g["scores"]), dev(g["boxes"]), dev(g["keep_idx"]))
    assert len(sc) == 40 and len(ck[1]) == 40 and float(sc.min()) >= np.sort(g["o_scores"])[-40]


@pytest.mark.parametrize("tag", ["n", "s"])
def test_rpn_outputs_and_proposals_equal_the_reference_fixture(m3d, golden, tag):
    """GPU RPN deltas / class response map vs the reference-run fixture (rpn_heads.py:94-116), and the reference's own
    deltas + scores pushed through the device proposal op reproduce the reference's rois and kept indices."""
    from m3d.model import DetectorM3D
    g = golden("prm_small_" + tag)
    stride, A = int(g["stride"]), int(g["A"])
    P = O.make_params(stride=stride, num_anchors=A, mlp_dim=64, seed=int(g["seed"]))
    cfg = O.Cfg(mlp_dim=64, score_thresh=0.0) if stride == 8 else O.Cfg.soma(mlp_dim=64)
    det = DetectorM3D({k: v.cuda() for k, v in P.items()}, cfg)
    feat = det.conv_body(dev(g["vol"]))
    prob, deltas = det.rpn(feat)
    assert np.allclose(feat.cpu().numpy(), g["feat"], rtol=1e-4, atol=1e-4)
    assert np.allclose(prob.cpu().numpy(), g["crm"], rtol=1e-4, atol=1e-5)
    assert np.allclose(deltas.cpu().numpy(), g["rpn_deltas"], rtol=1e-4, atol=1e-4)
    S, H, W = g["vol"].shape[-3:]
    info = np.array([S, H, W, 1.0])
    rois, probs, kidx = det.proposals(dev(g["crm"]), dev(g["rpn_deltas"]), info)
    flat = g["crm"][0].transpose(1, 2, 3, 0).ravel()
    if len(np.unique(flat)) == flat.size:                 # distinct scores: the reference's own result, bit for bit
        assert np.array_equal(kidx.cpu().numpy(), g["keep_idx"])
        assert np.allclose(rois.cpu().numpy(), g["rois"], rtol=2e-7, atol=1e-5)
    else:
        # the soma fixture's sigmoid saturates (several scores == 0.9999999): NumPy's unstable argsort()[::-1] leaves the
        # order of equal scores unspecified (SURVEY 8c caveat i), so the fixture's order is one of several valid ones; the
        # build's documented tie rule is checked against the oracle, and the fixture as a set of boxes scored the same
        r0, p0, k0 = O.generate_proposals_3d(g["crm"][0], g["rpn_deltas"][0], info, cfg.anchors, cfg.stride, cfg.pre_nms_topN,
                                             cfg.post_nms_topN, cfg.rpn_nms_thresh, cfg.rpn_min_size)
        assert np.array_equal(kidx.cpu().numpy(), k0) and np.allclose(rois.cpu().numpy(), r0, rtol=2e-7, atol=1e-5)
        both = np.intersect1d(kidx.cpu().numpy(), g["keep_idx"])
        assert len(both) >= 0.9 * len(g["keep_idx"])


# ------------------------------------------------------------------ RoIAlign adaptive sampling grid beyond the LDS tables
@pytest.mark.parametrize("res", [7, 3])
def test_roi_align_adaptive_grid_large_rois(m3d, res):
    """sampling_ratio = 0: grid = ceil(roi / res) per axis (roi_align_kernel_3d.cu:116-123).  RoIs of 100+ feature voxels need
    15-43 samples per bin - more than the kernels' LDS tables hold; they must be computed (reference order), not left zero."""
    rs = np.random.RandomState(11)
    f = rs.randn(2, 6, 40, 130, 140).astype(np.float32)
    rois = np.array([[0, 2.5, 3.0, 1.0, 133.0, 120.0, 38.0],       # x: grid 19 (res 7) -> 133 table entries
                     [1, 0.0, 0.0, 0.0, 139.0, 129.0, 39.0],       # whole map
                     [0, 10.0, 20.0, 5.0, 30.0, 40.0, 15.0],       # small: stays on the tabled path
                     [1, -50.0, -50.0, -20.0, 300.0, 300.0, 90.0],  # sticks out on every side
                     [0, 5.0, 5.0, 5.0, 110.0, 12.0, 9.0]], np.float32)   # one long axis only
    ref = O.roi_align_3d_forward(f, rois, res, res, res, 1.0, 0)
    assert np.abs(ref[[0, 1, 3, 4]]).max() > 0
    got = m3d.roi_align3d_forward(dev(f), dev(rois), res, res, res, 1.0, 0, exact=True).cpu().numpy()
    assert np.array_equal(got, ref)
    fast = m3d.roi_align3d_forward(dev(f), dev(rois), res, res, res, 1.0, 0).cpu().numpy()
    assert np.abs(fast - ref).max() <= 1e-5 * np.abs(f).max()
    roi_forward_within_its_bound(f, rois, res, 1.0, 0, fast)
    top = rs.randn(*ref.shape).astype(np.float32)
    gref = O.roi_align_3d_backward(top, rois, f.shape, res, res, res, 1.0, 0)
    ggot = m3d.roi_align3d_backward(dev(top), dev(rois), f.shape, res, res, res, 1.0, 0).cpu().numpy()
    assert np.allclose(ggot, gref, rtol=1e-4, atol=1e-5 * np.abs(gref).max())          # float atomics: order differs


def test_compact_rows_packs_the_valid_rows_of_every_item(m3d):
    """m3d_compact_rows = torch.cat([src[b, :counts[b]] for b]) with the counts read on the device: empty items, a full item, a count
    beyond the row capacity (clamped), 28-byte (RoI) and 8-byte (int64 index) rows; offsets = the exclusive prefix sums."""
    g = torch.Generator().manual_seed(5)
    B, rows = 6, 37
    counts = torch.tensor([5, 0, 37, 1, 50, 0], dtype=torch.int32)
    rois = torch.randn(B, rows, 7, generator=g)
    kidx = torch.randint(0, 1 << 40, (B, rows), generator=g)
    n = [min(int(c), rows) for c in counts]
    pr, offs = m3d.compact_rows(rois.cuda(), counts.cuda())
    pk, offs2 = m3d.compact_rows(kidx.cuda(), counts.cuda())
    total = sum(n)
    assert offs.cpu().tolist() == [0] + list(np.cumsum(n)) == offs2.cpu().tolist()
    assert torch.equal(pr[:total].cpu(), torch.cat([rois[b, :n[b]] for b in range(B)], 0))
    assert torch.equal(pk[:total].cpu(), torch.cat([kidx[b, :n[b]] for b in range(B)], 0))


def test_library_options_are_explicit(m3d):
    """include/m3d.h: no environment reads and NO mutable process-wide state in the release library - m3d_set_option refuses there; the
    tuning knobs live in the separate tuning build (libm3d_tune.so), loaded beside it by `with _lib.tuning()` and reset on exit."""
    from m3d import _lib
    assert _lib.lib().m3d_tuning_build() == 0                                  # the library the product path uses
    assert _lib.lib().m3d_set_option(b"xcd_map", 0) == -4                      # M3D_EUNSUPPORTED
    assert _lib.get_option("xcd_map") == 1 and _lib.get_option("tune_wino2") == -1
    assert _lib.get_option("tune_zw_grid") == -1 and _lib.lib().m3d_set_option(b"tune_zw_grid", 8) == -4
    with pytest.raises(m3d.M3DError):
        _lib.set_option("tune_stem", 4)
    x = torch.randn(1, 32, 8, 16, 64, device="cuda")
    w = torch.randn(64, 32, 3, 3, 3, device="cuda") * 0.05
    ref = m3d.PackedConv3d(w)(x)
    with _lib.tuning():
        assert _lib.lib().m3d_tuning_build() == 1
        conv = m3d.PackedConv3d(w)
        _lib.set_option("xcd_map", 0)
        a = conv(x)
        _lib.set_option("xcd_map", 1)
        b = conv(x)
        _lib.set_option("tune_stem", 4)
        _lib.set_option("tune_zw_grid", 8)
        assert _lib.get_option("tune_zw_grid") == 8
        with pytest.raises(m3d.M3DError):
            _lib.set_option("no_such_option", 1)
    assert torch.equal(a, b) and torch.equal(a, ref)  # the tile order is a speed option, never a result option
    assert _lib.lib().m3d_tuning_build() == 0
    with _lib.tuning():
        assert _lib.get_option("tune_stem") == -1 and _lib.get_option("xcd_map") == 1     # reset when the previous block ended
        assert _lib.get_option("tune_zw_grid") == -1


@pytest.mark.parametrize("shape", [(5, 6, 7), (64, 64, 64), (128, 128, 128)])
def test_norm1_on_device_equals_numpy(m3d, shape):
    """blob.py:179-184 (float32) and infer_simple.py:180-183 (float64 -> float32 crop) on the raw uint16 volume."""
    from m3d import tiling
    from m3d.synth import synth_volume
    im = synth_volume(7, shape) if shape[0] >= 64 else np.random.RandomState(0).randint(0, 900, shape).astype(np.uint16)
    im.flat[::97] = 0                                                    # masked-out voxels
    ref32 = tiling.norm1(im, np.float32).astype(np.float32)
    ref64 = tiling.norm1(im, np.float64)
    got32, st = m3d.norm1(dev(im), f32_arith=True, return_stats=True)
    got64 = m3d.norm1(dev(im), f32_arith=False)
    mask = im > 0
    assert abs(st[0].item() - im[mask].astype(np.float64).mean()) < 1e-9 * 100 and int(st[2].item()) == int(mask.sum())
    assert abs(st[1].item() - im[mask].astype(np.float64).std()) < 1e-9 * 100
    assert np.abs(got64.cpu().numpy() - ref64.astype(np.float32)).max() <= 1e-6      # one fp32 rounding of the same fp64 value
    assert np.abs(got32.cpu().numpy() - ref32).max() <= 2e-5                          # NumPy's fp32 pairwise mean/std vs exact
    f = m3d.norm1(dev(im.astype(np.float32)), f32_arith=True)
    assert torch.equal(f, got32)
    # a batch in one launch per pass: every volume with its own statistics, bit-identical to the one-volume calls
    im2 = (im.astype(np.int64) * 3 // 2 + 17).astype(np.uint16)
    b = m3d.norm1_batched(dev(np.stack([im, im2])), f32_arith=True)
    assert torch.equal(b[0], got32) and torch.equal(b[1], m3d.norm1(dev(im2), f32_arith=True))


# ------------------------------------------------------------------ box-head linear layers (fast_rcnn_heads.py:84-85,114-115,15-19)
@pytest.mark.parametrize("M,N,K,relu", [(1, 2, 32, False), (5, 14, 1024, False), (37, 64, 5488, True), (130, 128, 43904, True),
                                         (320, 1024, 87808, True), (1283, 1024, 1024, True), (257, 100, 1004, False)])
def test_linear_split_k_gemm_vs_fp64(m3d, M, N, K, relu):
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / np.sqrt(K)).cuda()
    b = torch.randn(N, generator=g).cuda()
    got = m3d.linear(x, w, b, relu=relu)
    ref = x.double() @ w.double().t() + b.double()
    if relu:
        ref = torch.relu(ref)
    scale = ref.abs().max().item()
    assert got.shape == (M, N) and (got.double() - ref).abs().max().item() <= 2e-6 * scale * max(1.0, np.sqrt(K / 1024.0))
    assert torch.equal(got, m3d.linear(x, w, b, relu=relu))              # deterministic (fixed-order split-K reduction)
    nb = m3d.linear(x, w, None, relu=False)
    assert (nb.double() - (x.double() @ w.double().t())).abs().max().item() <= 2e-6 * scale * max(1.0, np.sqrt(K / 1024.0))
    with pytest.raises(m3d.M3DError):
        m3d.linear(x[:, :K - 2].contiguous(), w[:, :K - 2].contiguous(), b)     # K % 4 != 0: unsupported, never silently wrong
    assert m3d.linear(x[:0], w, b).shape == (0, N)


@pytest.mark.parametrize("M,N,K,relu", [(1, 64, 32, False), (37, 64, 5504, True), (130, 128, 43904, True), (320, 1024, 87808, True),
                                         (1283, 1024, 1024, True), (257, 100, 1024, False), (1200, 1024, 87808, True), (1281, 256, 2048, True), (520, 128, 1024, False)])
def test_linear_bf16x3_split_gemm_is_as_accurate_as_the_fp32_kernel(m3d, M, N, K, relu):
    """Six bf16 MFMAs on the exact 3-way cut of both operands == fp32 accuracy: the error against fp64 stays within the same
    bound as the fp32 MFMA kernel's and within 2x of its measured error; awkward values (huge / tiny / negative) included."""
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g)
    x[0, :16] = torch.tensor([1e20, -1e20, 1e-20, -1e-20, 3.0, -3.0, 1.0000001, 0.99999994, 65504.0, 1e-30, 0.0, -0.0, 255.5, 1 / 3, 2 ** -100, 1.0])
    x = x.cuda()
    w = (torch.randn(N, K, generator=g) / np.sqrt(K)).cuda()
    w[0, :16] = torch.tensor([1e-20, 1e-20, 1e20, 1e20, 1 / 3, 1 / 7, 1.0, 1.0, 1e-4, 1e30, 5.0, 5.0, 1e-3, 3.0, 2 ** 100, -1.0]).cuda()
    b = torch.randn(N, generator=g).cuda()
    lin = m3d.SplitLinear(w, b)
    got = lin(x, relu=relu)
    ref = x.double() @ w.double().t() + b.double()
    if relu:
        ref = torch.relu(ref)
    scale = ref.abs().max().item()
    bound = 2e-6 * scale * max(1.0, np.sqrt(K / 1024.0))
    err = (got.double() - ref).abs().max().item()
    err32 = (m3d.linear(x, w, b, relu=relu).double() - ref).abs().max().item()
    assert got.shape == (M, N) and err <= bound and err <= 2.0 * err32 + 1e-7 * scale, (err, err32, bound)
    assert torch.equal(got, lin(x, relu=relu))                           # deterministic (whatever variant the shape selects)
    assert lin(x[:0]).shape == (0, N)
    for variant in ("packed", "w32"):                                    # 128 / 256 x 128 tiles on packed planes; 256 x 256 tiles, fp32 W cut in the kernel
        e = (lin(x, relu=relu, variant=variant).double() - ref).abs().max().item()
        assert e <= bound and e <= 2.0 * err32 + 1e-7 * scale, (variant, e, err32, bound)
    with pytest.raises(ValueError):
        m3d.SplitLinear(w[:, :K - 4].contiguous())                       # K % 32 != 0: the fp32 kernel's job
    # non-finite operands: every output fp32 makes non-finite is non-finite here too, and nothing else is (an inf operand comes out
    # as NaN: its cut is (inf, NaN, NaN) - documented in include/m3d.h; the box head never sees one unless the network diverged)
    xi = x.clone()
    xi[0, 20] = float("inf"); xi[min(1, M - 1), 21] = float("nan")
    if M > 2:
        xi[2, 22] = float("-inf")
    ref_i = xi @ w.t()
    for variant in ("packed", "w32"):
        got_i = lin(xi, variant=variant)
        assert torch.equal(torch.isfinite(got_i), torch.isfinite(ref_i)), variant


@pytest.mark.parametrize("M,N,K,relu", [(33, 64, 32, False), (37, 64, 5504, True), (130, 128, 43904, True), (320, 1024, 87808, True),
                                         (1283, 1024, 1024, True), (257, 100, 1024, False), (1253, 1024, 87808, True), (520, 128, 1024, False)])
def test_linear_f16x2_split_gemm_is_as_accurate_as_the_fp32_kernel(m3d, M, N, K, relu):
    """Three f16 MFMAs on the scaled two-way fp16 cut (22 bits) of both operands, against fp64 - on operands shaped like the layer's
    (x >= 0 with a heavy tail like a ReLU output and rows of different scale, kaiming weights), values down to 2^-17 of the largest
    and exact zeros mixed in, the bound given exactly, loosely (as the box head does: the feature map's) and swept from x.
    What is asserted: (a) the fp32 MFMA kernel's own acceptance bound (2e-6 of max|out| per sqrt(K / 1024)); (b) rms error <= 6e-7 of
    the product's rms - the cut leaves <= 3 x 2^-22 = 7e-7 per product with random sign, 2.5e-7 rms - or, where the fp32 accumulation
    itself rounds more than that (K = 87 808: 8e-7 in all three kernels), <= 1.5 x the fp32 kernel's rms error; (c) within 8 x the fp32 kernel's
    measured maximum: that kernel fuses every product into the accumulate (no product rounding) and, with K split over up to 64
    workgroups, adds short chains, so it beats BOTH this kernel and a sequential SGEMM (whose accumulation alone rounds by ~4e-6 of
    the result at K = 87 808); the claim here is "inside an SGEMM's error", not "as good as the split-K fp32 MFMA kernel"."""
    g = torch.Generator().manual_seed(M * 7 + N)
    x = torch.relu(torch.randn(M, K, generator=g)) * torch.exp(torch.randn(M, 1, generator=g))
    x[0, :8] = torch.tensor([37.5, 1e-4, 3.0, 0.0, 1.0000001, 0.99999994, 255.5, 1 / 3])
    x = x.cuda()
    w = (torch.randn(N, K, generator=g) / np.sqrt(K)).cuda()
    w[0, :8] = torch.tensor([1 / 3, 1 / 7, 1.0, 1.0, 1e-4, -2e-5, 5.0, -1.0]).cuda() * float(w.abs().max())
    b = torch.randn(N, generator=g).cuda()
    lin = m3d.ops.SplitLinearF16(w, b)
    ref = x.double() @ w.double().t() + b.double()
    if relu:
        ref = torch.relu(ref)
    scale = ref.abs().max().item()
    prod_rms = (x.double() @ w.double().t()).pow(2).mean().sqrt().item()
    bound = 2e-6 * scale * max(1.0, np.sqrt(K / 1024.0))
    g32 = m3d.linear(x, w, b, relu=relu)
    err32 = (g32.double() - ref).abs().max().item()
    rms32 = (g32.double() - ref).pow(2).mean().sqrt().item()
    xb = m3d.ops.absmax(x)
    assert float(xb) == float(x.abs().max())
    for xbound in (xb, xb * 200.0, None):                                # exact bound, a loose one (a feature map's), swept inside the call
        got = lin(x, relu=relu, x_bound=xbound)
        err = (got.double() - ref).abs().max().item()
        rms = (got.double() - ref).pow(2).mean().sqrt().item()
        assert got.shape == (M, N) and err <= bound and err <= 8.0 * err32 + 1e-7 * scale, (err, err32, bound)
        # long K: the accumulation's rounding dominates in both kernels; this one's chains are longer (256 x 256 tiles split K 12 ways at
        # M = 1253, the fp32 kernel's 128 x 128 tiles about twice as often): 1.27 x measured there
        assert rms <= max(6e-7 * prod_rms, 1.5 * rms32), (rms, prod_rms, rms32)
        assert torch.equal(got, lin(x, relu=relu, x_bound=xbound))       # deterministic
    assert lin(x[:0]).shape == (0, N)
    with pytest.raises(ValueError):
        m3d.ops.SplitLinearF16(w[:, :K - 4].contiguous())                # K % 32 != 0: the fp32 kernel's job
    # all-zero x (no RoI feature survives the ReLU): the bias, exactly
    z = lin(torch.zeros_like(x), relu=False)
    assert torch.equal(z, b.expand(M, N))


# ------------------------------------------------------------------ batched, fused box stages (csrc/box_fused.hip)
def test_fused_proposals_without_nms_keep_every_valid_box(m3d):
    """RPN_NMS_THRESH <= 0: the reference applies post_nms_topN only inside `if nms_thresh > 0`
    (lib/modeling/generate_proposals_3d.py:167-171), so every box that passes the size filter is kept - fused launch, per-tile
    entry point and oracle agree row for row although post_nms_topN < pre_nms_topN."""
    rs = np.random.RandomState(21)
    B, A, S, H, W = 2, 35, 8, 8, 8
    cfg = O.Cfg()
    sc = rs.uniform(0, 1, (B, A, S, H, W)).astype(np.float32)
    dl = (rs.randn(B, 6 * A, S, H, W) * 0.2).astype(np.float32)
    info = np.array([64., 64., 64., 1.0])
    pre, post = 600, 100
    rois, probs, kidx, num = m3d.generate_proposals3d_batched(dev(sc), dev(dl), cfg.anchors, 8., info, pre, post, 0.0)
    assert rois.shape[1] == pre
    for b in range(B):
        r0, p0, k0 = O.generate_proposals_3d(sc[b], dl[b], info, cfg.anchors, 8, pre, post, 0.0, 0)
        n = int(num[b])
        assert n == len(k0) and n > post
        assert np.array_equal(kidx[b, :n].cpu().numpy(), k0)
        assert np.array_equal(probs[b, :n].cpu().numpy(), p0.ravel())
        assert np.allclose(rois[b, :n, 1:].cpu().numpy(), r0[:, 1:], rtol=2e-7, atol=1e-5)
        r1, p1, k1 = m3d.generate_proposals3d(dev(sc[b]), dev(dl[b]), cfg.anchors, 8., info, pre, post, 0.0)
        assert torch.equal(k1, kidx[b, :n]) and torch.equal(r1[:, 1:], rois[b, :n, 1:])


def test_fused_box_results_ignore_rows_beyond_the_declared_maximum(m3d):
    """Offsets contract of m3d_box_results3d_batched (include/m3d.h): an item with more rows than max_rows_per_item has its
    surplus rows ignored - nothing is written outside the item's own outputs (the neighbouring item stays exact)."""
    rs = np.random.RandomState(5)
    nc, cap = 2, 64
    rows = [100, 40]                                              # item 0 breaks the contract, item 1 does not
    R = sum(rows)
    scores = rs.uniform(0, 1, (R, nc)).astype(np.float32)
    ctr = rs.uniform(10, 50, (R, 3)); half = rs.uniform(2, 6, (R, 3))
    one = np.hstack((ctr - half, ctr + half)).astype(np.float32)
    boxes = np.tile(one, (1, nc))
    off = torch.tensor([0, rows[0], R], dtype=torch.int32, device="cuda")
    cb, ck, cnt = m3d.box_results3d_batched(dev(scores), dev(boxes), None, off, nc, 0.05, 0.3, 300, cap)
    # item 1 alone, within the contract
    off1 = torch.tensor([0, rows[1]], dtype=torch.int32, device="cuda")
    cb1, ck1, cnt1 = m3d.box_results3d_batched(dev(scores[rows[0]:]), dev(boxes[rows[0]:]), None, off1, nc, 0.05, 0.3, 300, cap)
    assert torch.equal(cnt[1], cnt1[0])
    n1 = int(cnt1[0, 1])
    assert torch.equal(cb[1, 1, :n1], cb1[0, 1, :n1])
    # item 0 = its first `cap` rows
    off0 = torch.tensor([0, cap], dtype=torch.int32, device="cuda")
    cb0, ck0, cnt0 = m3d.box_results3d_batched(dev(scores[:cap]), dev(boxes[:cap]), None, off0, nc, 0.05, 0.3, 300, cap)
    assert torch.equal(cnt[0], cnt0[0])
    n0 = int(cnt0[0, 1])
    assert torch.equal(cb[0, 1, :n0], cb0[0, 1, :n0])


def test_fused_proposals_batched_bit_exact_with_oracle_and_golden(m3d, golden):
    """One launch for a batch of tiles == the per-tile reference op, item by item: kept flat indices, probabilities and row
    order bit for bit (incl. saturated ties), boxes to one fp32 ulp; fixtures of the reference's own GenerateProposalsOp_3d."""
    g = golden("proposals")
    for tag, sizes, ratios in (("n", (10, 27, 33, 38, 42, 46, 50), [[1.0, 0.5], [0.5, 0.5], [2., 0.5], [0.2, 0.5], [3., 2.]]),
                               ("s", (10, 12, 14, 16, 18, 20, 22, 24, 28, 30, 34, 36, 38, 40), [[1.0, 1.0]])):
        stride = float(g[tag + "_stride"])
        anchors = O.generate_anchors_3d(stride, sizes, ratios)
        rois, probs, kidx, num = m3d.generate_proposals3d_batched(dev(g[tag + "_scores"]), dev(g[tag + "_deltas"]), anchors, stride,
                                                                  g[tag + "_im_info"][0], int(g["pre"]), int(g["post"]), float(g[tag + "_thr"]))
        n = int(num[0])
        assert np.array_equal(kidx[0, :n].cpu().numpy(), g[tag + "_keep_idx"])
        assert np.array_equal(probs[0, :n].cpu().numpy()[:, None], g[tag + "_probs"])
        assert np.allclose(rois[0, :n].cpu().numpy(), g[tag + "_rois"], rtol=2e-7, atol=1e-5)
    rs = np.random.RandomState(8)
    B, A, S, H, W = 3, 35, 16, 16, 16
    cfg = O.Cfg()
    sc = rs.uniform(0, 1, (B, A, S, H, W)).astype(np.float32)
    sc[rs.uniform(0, 1, sc.shape) > 0.995] = 1.0                   # saturated sigmoid: exact ties at the top
    sc[2] = np.round(sc[2], 2)                                     # item 2: ties everywhere
    dl = (rs.randn(B, 6 * A, S, H, W) * 0.2).astype(np.float32)
    info = np.array([128., 128., 128., 1.0])
    rois, probs, kidx, num = m3d.generate_proposals3d_batched(dev(sc), dev(dl), cfg.anchors, 8., info, 1000, 1000, 0.15, first_batch_index=5)
    for b in range(B):
        r0, p0, k0 = O.generate_proposals_3d(sc[b], dl[b], info, cfg.anchors, 8, 1000, 1000, 0.15, 0)
        n = int(num[b])
        assert n == len(k0) and np.array_equal(kidx[b, :n].cpu().numpy(), k0), b
        assert np.array_equal(probs[b, :n].cpu().numpy(), p0.ravel())
        got = rois[b, :n].cpu().numpy()
        assert np.all(got[:, 0] == 5 + b) and np.allclose(got[:, 1:], r0[:, 1:], rtol=2e-7, atol=1e-5)
        # and the multi-launch per-tile entry point gives the very same rows
        r1, p1, k1 = m3d.generate_proposals3d(dev(sc[b]), dev(dl[b]), cfg.anchors, 8., info, 1000, 1000, 0.15)
        assert torch.equal(k1, kidx[b, :n]) and torch.equal(r1[:, 1:], rois[b, :n, 1:])
    # far more exact ties at the threshold than the select's LDS candidate list holds (4096): the radix passes go on over the
    # flat-index digits of the bucket's list; and a map with fewer anchors than pre_nms_topN above... (everything selected)
    sc2 = np.full((2, A, S, H, W), 0.5, np.float32)
    sc2[0].reshape(-1)[rs.permutation(A * S * H * W)[:300]] = 0.75
    sc2[1, :, :, :, 8:] = 0.25
    rois, probs, kidx, num = m3d.generate_proposals3d_batched(dev(sc2), dev(dl[:2]), cfg.anchors, 8., info, 1000, 1000, 0.15)
    for b in range(2):
        r0, p0, k0 = O.generate_proposals_3d(sc2[b], dl[b], info, cfg.anchors, 8, 1000, 1000, 0.15, 0)
        n = int(num[b])
        assert n == len(k0) and np.array_equal(kidx[b, :n].cpu().numpy(), k0), b
        assert np.array_equal(probs[b, :n].cpu().numpy(), p0.ravel())
    small = rs.uniform(0, 1, (1, A, 2, 3, 2)).astype(np.float32)                       # 420 anchors < pre_nms_topN
    dsm = (rs.randn(1, 6 * A, 2, 3, 2) * 0.2).astype(np.float32)
    rois, probs, kidx, num = m3d.generate_proposals3d_batched(dev(small), dev(dsm), cfg.anchors, 8., np.array([16., 24., 16., 1.0]), 1000, 1000, 0.15)
    r0, p0, k0 = O.generate_proposals_3d(small[0], dsm[0], np.array([16., 24., 16., 1.0]), cfg.anchors, 8, 1000, 1000, 0.15, 0)
    n = int(num[0])
    assert n == len(k0) and np.array_equal(kidx[0, :n].cpu().numpy(), k0)
    # pre_nms_topN beyond one workgroup's capacity is refused, never truncated
    with pytest.raises(m3d.M3DError):
        m3d.generate_proposals3d_batched(dev(sc), dev(dl), cfg.anchors, 8., info, 6000, 1000, 0.15)


def test_fused_box_results_and_batched_nms_vs_oracle(m3d):
    """box_results_with_nms_and_limit for three tiles of different sizes in one launch (score threshold, per-class NMS, cap
    semantics, kept indices) and the batched NMS + pack, against the oracle item by item - with heavy score ties."""
    rs = np.random.RandomState(12)
    sizes = [400, 1, 777]
    nc = 3
    scores, boxes, keep = [], [], []
    for R in sizes:
        s = np.round(rs.uniform(0, 1, (R, nc)), 2).astype(np.float32)
        c = rs.uniform(0, 100, (R, nc, 3)); e = rs.uniform(4, 40, (R, nc, 3))
        scores.append(s); boxes.append(np.concatenate((c - e / 2, c + e / 2), 2).reshape(R, 6 * nc).astype(np.float32))
        keep.append(rs.permutation(100000)[:R].astype(np.int64))
    offs = np.concatenate(([0], np.cumsum(sizes))).astype(np.int32)
    S, Bx, Kp = np.vstack(scores), np.vstack(boxes), np.concatenate(keep)
    for cap_im in (300, 40, 0):
        cb, ck, cnt = m3d.box_results3d_batched(dev(S), dev(Bx), dev(Kp), dev(offs), nc, 0.05, 0.15, cap_im, max(sizes))
        cnt = cnt.cpu().numpy()
        for b, R in enumerate(sizes):
            sc, bx, cls_boxes, cls_keep = O.box_results_with_nms_and_limit(scores[b], boxes[b], keep[b], num_classes=nc, score_thresh=0.05,
                                                                           nms_thresh=0.15, detections_per_im=cap_im)
            assert cnt[b, 0] == 0
            for j in range(1, nc):
                n = cnt[b, j]
                assert n == len(cls_boxes[j]), (cap_im, b, j)
                assert np.array_equal(cb[b, j, :n].cpu().numpy(), cls_boxes[j]) and np.array_equal(ck[b, j, :n].cpu().numpy(), cls_keep[j])
    # batched NMS + pack: items of different length inside one padded tensor, by score and by volume
    n_items, cap_in = 4, 900
    dets = np.zeros((n_items, cap_in, 7), np.float32)
    counts = np.array([900, 0, 65, 300], np.int32)
    for b in range(n_items):
        c = rs.uniform(0, 100, (cap_in, 3)); e = rs.uniform(4, 40, (cap_in, 3))
        dets[b] = np.hstack((c - e / 2, c + e / 2, np.round(rs.uniform(0, 1, (cap_in, 1)), 2)))
    for by_vol in (False, True):
        r = m3d.nms3d_batched(dev(dets), dev(counts), 0.2, by_volume=by_vol, pack_cap=300)
        for b in range(n_items):
            d = dets[b, :counts[b]]
            ref = (O.nms_3d_volume if by_vol else O.nms_3d)(d, 0.2) if counts[b] else np.zeros((0,), np.int64)
            n = int(r["num"][b])
            assert n == len(ref) and np.array_equal(r["keep"][b, :n].cpu().numpy(), ref)
            p = r["packed"][b].cpu().numpy()
            m = min(n, 300)
            assert p[300, 0] == m and np.array_equal(p[:m], d[ref[:m]]) and not p[m:300].any() and not p[300, 1:].any()


def test_rpn_heads_conv_with_sigmoid_and_split_equals_the_three_launches(m3d):
    """m3d_conv3d_forward_split_sigmoid (one launch) == the 1x1x1 conv of the concatenated heads + torch.sigmoid of the first A channels +
    the two slice copies it replaces (rpn_heads.py:96-98,116): bit for bit, on a ragged map and a batch."""
    for B, Cc, A, shp in ((1, 128, 14, (5, 9, 13)), (3, 256, 35, (4, 8, 24)), (2, 64, 3, (2, 3, 70))):
        g = torch.Generator().manual_seed(A)
        x = torch.randn((B, Cc) + shp, generator=g).cuda()
        w = (torch.randn(7 * A, Cc, 1, 1, 1, generator=g) * 0.2).cuda()
        b = torch.randn(7 * A, generator=g).cuda()
        conv = m3d.PackedConv3d(w)
        o = conv(x, shift=b)
        prob, deltas = conv.split_sigmoid(x, A, shift=b)
        assert prob.shape == (B, A) + shp and deltas.shape == (B, 6 * A) + shp and prob.is_contiguous() and deltas.is_contiguous()
        assert torch.equal(deltas, o[:, A:])
        assert torch.equal(prob, torch.sigmoid(o[:, :A]))          # the same formula on the same device exp: identical bits


def test_box_head_outputs_equals_softmax_and_the_decode_kernel(m3d):
    """m3d_box_head_outputs (one launch) == torch.softmax of the class scores + the raw deltas + m3d_bbox_transform3d with the clip
    (fast_rcnn_heads.py:42-45, core/test.py:250-251): bit for bit for nc = 2 (both shipped configs), 1e-7 for nc = 3."""
    for M, nc in ((1, 2), (333, 2), (1281, 2), (77, 3)):
        g = torch.Generator().manual_seed(M)
        outs = (torch.randn(M, 7 * nc, generator=g) * 2).cuda()
        rois = torch.rand(M, 7, generator=g) * 100
        rois[:, 4:] = rois[:, 1:4] + 1 + rois[:, 4:] * 0.3
        rois = rois.cuda()
        wts = (10., 10., 10., 5., 5., 5.)
        cls, bbox, pred = m3d.box_head_outputs(outs, rois, nc, wts, clip_to=(64, 200, 200))
        ref_cls = torch.softmax(outs[:, :nc].contiguous(), dim=1)
        ref_bbox = outs[:, nc:].contiguous()
        ref_pred = m3d.bbox_transform3d(rois[:, 1:7].contiguous(), ref_bbox, wts, clip_to=(64, 200, 200))
        assert torch.equal(bbox, ref_bbox) and torch.equal(pred, ref_pred)
        if nc == 2:
            assert torch.equal(cls, ref_cls)
        else:
            assert torch.allclose(cls, ref_cls, rtol=0, atol=3e-7)        # three terms: the summation order may differ
        _, _, unclipped = m3d.box_head_outputs(outs, rois, nc, wts)
        assert torch.equal(unclipped, m3d.bbox_transform3d(rois[:, 1:7].contiguous(), ref_bbox, wts))


def test_compact_rows2_packs_both_sets_and_mirrors_the_counts(m3d):
    B, rows = 5, 40
    g = torch.Generator().manual_seed(1)
    a = torch.randn(B, rows, 7, generator=g).cuda()
    k = torch.randint(0, 1 << 40, (B, rows), generator=g).cuda()
    counts = torch.tensor([3, 0, 40, 17, 99], dtype=torch.int32).cuda()           # 99 is clamped to the row count
    host = torch.zeros((B,), dtype=torch.int32).pin_memory()
    pa, pk, offs = m3d.compact_rows2(a, k, counts, host)
    torch.cuda.synchronize()
    n = [3, 0, 40, 17, 40]
    assert host.tolist() == n and offs.cpu().tolist() == [0, 3, 3, 43, 60, 100]
    assert torch.equal(pa[:100], torch.cat([a[b, :n[b]] for b in range(B)])) and torch.equal(pk[:100], torch.cat([k[b, :n[b]] for b in range(B)]))
    p1, o1 = m3d.compact_rows(a, counts)
    assert torch.equal(p1[:100], pa[:100]) and torch.equal(o1, offs)


@pytest.mark.parametrize("R,C,shape", [(37, 32, (6, 9, 11)), (300, 64, (8, 12, 12)), (70, 256, (4, 5, 6))])
def test_fc1_with_the_roialign_gather_in_its_operand_loader_equals_the_two_launch_path(m3d, R, C, shape):
    """SURVEY 8f-1's fused variant (m3d_linear_bf16x3_roi_forward: the GEMM computes its A operand from the feature maps) against the
    product path it was measured against (RoIAlign3D, then the bf16x3 GEMM): the same samples and weights in another summation order -
    the GEMM inputs agree to 1e-6 of max|x|, the outputs to 1e-5 of max|out|.  RoIs sticking out of the map, batch indices, zero-size."""
    g = torch.Generator().manual_seed(R)
    B = 2
    S, H, W = shape
    feat = torch.randn((B, C) + shape, generator=g).cuda()
    lo = torch.rand(R, 3, generator=g) * torch.tensor([W * 8.0, H * 8.0, S * 8.0]) - 6.0
    sz = torch.rand(R, 3, generator=g) * 30.0 + 1.0
    rois = torch.cat([torch.randint(0, B, (R, 1), generator=g).float(), lo, lo + sz], 1)
    rois[0, 4:] = rois[0, 1:4]                                      # a zero-size RoI (clamped to one voxel by the reference rule)
    rois[1, 1:4] = -100.0; rois[1, 4:] = -90.0                      # a RoI wholly outside: every sample invalid -> zeros
    rois = rois.cuda()
    w = (torch.randn(128, C * 343, generator=g) / (C * 343) ** 0.5).cuda()
    b = torch.randn(128, generator=g).cuda()
    lin = m3d.SplitLinear(w, b)
    x = m3d.roi_align3d_forward(feat, rois, 7, 7, 7, 0.125, 2).view(R, -1)
    ref = lin(x, relu=True, variant="packed")
    got = m3d.linear_roi_fused(lin, feat, rois, 0.125, relu=True)
    assert float(x[1].abs().max()) == 0.0
    assert (got - ref).abs().max().item() <= 1e-5 * ref.abs().max().item() + 1e-6
    # and against the ORACLE, not only against the library's own two-launch path: the oracle's RoIAlign3D (the line-by-line restatement of
    # roi_align_kernel_3d.cu:81-151, incl. its (y, x, z) memory order) followed by a float64 linear + ReLU (fast_rcnn_heads.py:114)
    xo = O.roi_align_3d_forward(feat.cpu().numpy(), rois.cpu().numpy(), 7, 7, 7, 0.125, 2).reshape(R, -1)
    ref64 = np.maximum(xo.astype(np.float64) @ w.cpu().numpy().astype(np.float64).T + b.cpu().numpy().astype(np.float64), 0.0)
    scale = float(np.abs(ref64).max())
    assert float(np.abs(got.cpu().numpy().astype(np.float64) - ref64).max()) <= 2e-5 * scale + 1e-6
    assert float(np.abs(ref.cpu().numpy().astype(np.float64) - ref64).max()) <= 2e-5 * scale + 1e-6
    # the workspace query covers the plan the fused entry point really launches (small M re-plans to the 256-row tile)
    from m3d._lib import lib
    for M_ in (1, 7, R, 300, 1200):
        assert lib().m3d_linear_bf16x3_roi_workspace_bytes(M_, 128, C * 343) >= 16


@pytest.mark.parametrize("cin,cout,shape,batch", [(32, 64, (8, 20, 36), 1), (64, 64, (5, 9, 17), 2), (16, 128, (4, 4, 16), 1), (128, 96, (7, 13, 21), 1),
                                                  (64, 256, (8, 25, 25), 1), (48, 64, (6, 10, 20), 1), (80, 32, (3, 5, 33), 3)])
def test_bf16x3_direct_conv_has_fp32_accuracy_and_the_fp32_kernels_exact_zeros(cin, cout, shape, batch):
    """m3d_conv3d_x3_forward (three-way bf16 cut of both operands, six bf16 MFMA products per fp32 product) as the PRM norm conv
    N = conv3d(X - min X, relu(W), padding 1) (peak_backprop_3d.py:37-44): against float64 its error is the fp32-MFMA kernel's; ragged
    tiles in all three axes, a channel count that is not a multiple of the 64-channel tile, batches; and where the inputs under every
    positive weight are zero the result is exactly 0.0 - the same voxels as the fp32 kernel's (the backward's `N < 1e-10` test)."""
    import m3d
    from m3d import ops
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.rand((batch, cin) + shape, generator=g) * (torch.rand((batch, cin) + shape, generator=g) > 0.3)
    x = x + 0.25
    x[:, :, : max(3, shape[0] // 2), : max(3, shape[1] // 2)] = 0.25          # a constant block at the minimum: exact zeros after the shift
    w = torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.1
    xc, wc = x.cuda(), w.cuda()
    off = ops.reduce_min(xc)
    assert float(off) == 0.25
    got = ops.X3Conv3d(wc, ops.W_RELU)(xc, in_offset=off).cpu()
    f32 = ops.PackedConv3d(wc, ops.W_RELU)(xc, in_offset=off).cpu()
    ref = torch.nn.functional.conv3d((x - 0.25).double(), torch.relu(w).double(), padding=1)
    scale = float(ref.abs().max())
    e_x3, e_f32 = float((got.double() - ref).abs().max()) / scale, float((f32.double() - ref).abs().max()) / scale
    assert e_x3 < 4e-6 and e_x3 <= max(3.0 * e_f32, 1e-6), (e_x3, e_f32)
    zero = ref == 0
    assert int(zero.sum()) > 0
    assert torch.equal(got == 0, zero) and torch.equal(f32 == 0, zero)
    # without a workspace the library runs every workgroup over all of K (no split): same sums in another order
    import ctypes as C
    from m3d._lib import lib, check
    conv = ops.X3Conv3d(wc, ops.W_RELU)
    whole = torch.empty_like(got, device="cuda")
    check(lib().m3d_conv3d_x3_forward(C.c_void_p(xc.data_ptr()), C.c_void_p(conv.packed.data_ptr()), C.c_void_p(whole.data_ptr()), batch, cin, cout,
                                      shape[0], shape[1], shape[2], C.c_void_p(off.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "x3")
    assert float((whole.cpu().double() - ref).abs().max()) / scale < 4e-6 and torch.equal(whole.cpu() == 0, zero)
    plain = ops.X3Conv3d(wc, ops.W_PLAIN)(xc).cpu()                          # signed weights, no offset
    ref2 = torch.nn.functional.conv3d(x.double(), w.double(), padding=1)
    assert float((plain.double() - ref2).abs().max()) / float(ref2.abs().max()) < 2e-6
    # round 6: the f16x2 split (two scaled fp16 pieces per operand, three products): on these inputs (every operand >= 0.25 above the
    # minimum or exactly at it) the same exact zeros - the fp32 kernel's zeros stay zero, and no operand is small enough to cut to 0 (in
    # general one below its bound x 2^-39 does: tests/test_gpu_f16x2_range.py) - error against fp64 within 3e-6 of the largest output,
    # minima / maxima from the two-launch sweep, with and without the K split
    mn, mx = ops.reduce_minmax_multi([xc, xc[:, :1].contiguous()])
    assert float(mn[0]) == float(x.min()) == 0.25 and float(mx[0]) == float(x.max()) and float(mx[1]) == float(x[:, :1].max())
    c16 = ops.X3Conv3d(wc, ops.W_RELU, f16=True)
    got16 = c16(xc, in_offset=off, in_max=mx[0:1]).cpu()
    e16 = float((got16.double() - ref).abs().max()) / scale
    assert e16 < 3e-6, (e16, e_f32)
    assert torch.equal(got16 == 0, zero) and bool((got16 >= 0).all())
    whole16 = torch.empty_like(got, device="cuda")
    check(lib().m3d_conv3d_x3f_forward_ws(C.c_void_p(xc.data_ptr()), C.c_void_p(c16.packed.data_ptr()), C.c_void_p(whole16.data_ptr()), batch, cin, cout,
                                          shape[0], shape[1], shape[2], C.c_void_p(off.data_ptr()), C.c_void_p(mx.data_ptr()), None, C.c_size_t(0),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "x3f")
    assert float((whole16.cpu().double() - ref).abs().max()) / scale < 3e-6 and torch.equal(whole16.cpu() == 0, zero)
    p16 = ops.X3Conv3d(wc, ops.W_PLAIN, f16=True)(xc, in_max=ops.absmax(xc)).cpu()      # signed weights, no offset: bound = max |x|
    assert float((p16.double() - ref2).abs().max()) / float(ref2.abs().max()) < 3e-6
    with pytest.raises(ValueError):
        c16(xc, in_offset=off)                                               # the f16 form needs the operand's bound


def test_reduce_min_multi_equals_the_single_array_minima(m3d):
    """m3d_reduce_min_multi (every `input.min()` of a PRM forward in two launches): up to 12 arrays of any size / alignment, each minimum
    bit-equal to torch's and to the single-array entry point."""
    g = torch.Generator().manual_seed(5)
    sizes = [1, 3, 4, 257, 4096, 65537, 1 << 20, 12345, 64, 999999, 31, 2048]
    base = torch.randn(sum(sizes) + 7, generator=g).cuda()
    xs, o = [], 3                                              # views at odd offsets: not 16-byte aligned
    for n in sizes:
        xs.append(base[o:o + n]); o += n
    got = m3d.ops.reduce_min_multi(xs).cpu()
    assert got.shape == (12,)
    for i, x in enumerate(xs):
        assert float(got[i]) == float(x.min()) == float(m3d.reduce_min(x.contiguous()))
    assert float(m3d.ops.reduce_min_multi(xs[:1])[0]) == float(xs[0].min())
    # beyond the entry point's 12 arrays the host op runs groups of 12 (a deeper backbone must not turn the PRM forward into an error);
    # the C entry point itself still refuses 13
    many = xs + xs[::-1] + xs[:5]                              # 29 arrays: groups of 12 + 12 + 5
    gm = m3d.ops.reduce_min_multi(many).cpu()
    assert gm.shape == (29,)
    for i, x in enumerate(many):
        assert float(gm[i]) == float(x.min())
    import ctypes as C
    n = 13
    ptrs = (C.c_void_p * n)(*[x.data_ptr() for x in many[:n]])
    cnts = (C.c_int64 * n)(*[x.numel() for x in many[:n]])
    out = torch.empty((n,), device="cuda")
    wsb = m3d._lib.lib().m3d_reduce_min_multi_workspace_bytes()
    ws = torch.empty((wsb,), dtype=torch.uint8, device="cuda")
    rc = m3d._lib.lib().m3d_reduce_min_multi(ptrs, cnts, n, C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(wsb), None)
    assert rc == -1                                            # M3D_EINVAL


@pytest.mark.parametrize("shape", [(5, 7, 9), (6, 10, 14), (3, 5, 8)])
def test_prm_scatter_fills_maps_whose_voxel_count_is_not_a_multiple_of_four(m3d, shape):
    """m3d_prm_scatter writes every voxel of [P,D,H,W] (zero outside the window, NaN everywhere for a zero-sum peak): maps of 315 / 840 /
    120 voxels - odd counts take the dword fill over a (chunks, peak) grid - against the statement in NumPy, bit for bit."""
    rng = np.random.RandomState(11)
    Pn, wn = 5, 4
    D, H, W = shape
    win = torch.from_numpy(rng.rand(Pn, wn, wn, wn).astype(np.float32)).cuda()
    sums = win.sum((1, 2, 3))
    sums[3] = 0.0
    org = torch.from_numpy(rng.randint(-2, 4, (Pn, 3)).astype(np.int32)).cuda()
    got = m3d.prm_scatter(win, sums, org, shape).cpu().numpy()
    ref = np.zeros((Pn, D, H, W), np.float32)
    wh, sh, oh = win.cpu().numpy(), sums.cpu().numpy(), org.cpu().numpy()
    for p in range(Pn):
        ref[p] = np.float32(0) / sh[p] if sh[p] == 0 else 0.0
        for z in range(wn):
            for y in range(wn):
                for x in range(wn):
                    q = oh[p] + (z, y, x)
                    if 0 <= q[0] < D and 0 <= q[1] < H and 0 <= q[2] < W:
                        ref[p, q[0], q[1], q[2]] = wh[p, z, y, x] / sh[p]
    assert np.array_equal(got, ref, equal_nan=True)


def test_paint_begin_fills_the_sentinel_and_derives_the_ids(m3d):
    """m3d_paint_begin: label volume at 0xFFFFFFFF, present flags at 0, ids = idx + first_id where both stages succeeded and the
    detection's map has a non-zero voxel, else -1 (binarization_soma.py:66,74-76,94-98) - one launch for seven element-wise ones."""
    from m3d import ops
    R, P = 9, 14
    idx = torch.tensor([0, 2, 3, 5, 6, 8, 9, 12, 13], dtype=torch.int64).cuda()
    st_o = torch.tensor([0, 0, 1, 0, 3, 0, 0, 0, 2], dtype=torch.int32).cuda()
    st_c = torch.tensor([0, 1, 0, 0, 0, 2, 0, 0, 0], dtype=torch.int32).cuda()
    stats = torch.zeros((P, 4), dtype=torch.int32)
    stats[:, 3] = torch.tensor([1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 7, 1])          # map 9 is all zero
    stats = stats.cuda()
    for shape in ((5, 6, 8), (3, 5, 7)):                       # voxel counts divisible by 4 and not
        vol, present, ids = ops.paint_begin(shape, 5 + P, st_o, st_c, stats, idx, 5, "cuda")
        assert vol.dtype == torch.int32 and tuple(vol.shape) == shape and bool((vol == -1).all())
        assert present.dtype == torch.uint8 and present.numel() == 5 + P and not bool(present.any())
        assert ids.cpu().tolist() == [5, -1, -1, 10, -1, -1, -1, 17, -1]
        _, _, ids2 = ops.paint_begin(shape, 5 + P, st_o, st_c, None, idx, 5, "cuda")            # no map statistics: maps count as non-empty
        assert ids2.cpu().tolist() == [5, -1, -1, 10, -1, -1, 14, 17, -1]


def test_upload_packed_is_one_copy_with_the_arrays_values(m3d):
    from m3d import ops
    rs = np.random.RandomState(3)
    arrs = [rs.randint(0, 1 << 40, (17,)).astype(np.int64), rs.randint(0, 99, (17, 6)).astype(np.int32), rs.randint(0, 9, (17, 3)).astype(np.int32),
            np.zeros((0,), np.int32), rs.rand(5).astype(np.float32), rs.randint(0, 255, (3,)).astype(np.uint8)]
    outs = ops.upload_packed(arrs, "cuda")
    torch.cuda.synchronize()
    for a, t in zip(arrs, outs):
        assert tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy(), a)
        assert t.numel() == 0 or t.data_ptr() % 16 == 0
