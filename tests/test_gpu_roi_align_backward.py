"""GPU: the RoIAlign3D backward (csrc/roi_align3d.hip: roi_align3d_kernel<true>, roi_untabled_range<true>) and the autograd wrappers of
m3d.compat against the fp64 reference of tests/roi_align_backward_cases.py, element by element, over its case table (what each case
reaches - channel chunks, loop trips, tabled / untabled path, the classes of samples - is proved on the CPU by
tests/test_roi_align_backward_cases_host.py, which also shows that the bound rejects five wrong backwards).

 (a) every case: every element within (n_e + 8) * 2^-24 * A_e of the reference, exactly 0.0 where no add lands; the largest err / bound
     and its element are in the assertion message and printed (pytest -s), the worst per case again at the end of the module;
 (b) top == 0 gives an all-zero gradient; the gradient of 2 * top is twice the gradient of top within the bounds of the two sides
     (doubling is exact in fp32, so only the order of the atomic adds separates them);
 (c) RoIAlign_3d / RoIAlignAvg_3d / RoIAlignMax_3d: features.grad within the bound of the reference applied to the grad_output the
     Function received, a non-contiguous upstream gradient, no gradient for the RoIs;
 (d) the refused configuration (7^3 bins at a fixed ratio of 10) raises and writes nothing."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_align_backward_cases as T

pytestmark = pytest.mark.gpu

WORST = {}


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    yield _m
    for cid, r in WORST.items():
        print("RoIAlign3D backward: largest |got - ref| / bound  %-18s %.4f" % (cid, r))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the table's arrays are read-only


def backward(m3d, c, top):
    return m3d.roi_align3d_backward(dev(top), dev(T.rois(c)), c.shape, c.bins[0], c.bins[1], c.bins[2], c.scale, c.ratio).cpu().numpy()


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_kernel_against_fp64(m3d, c):
    res = T.reference_of(c)
    got = backward(m3d, c, T.top(c))
    assert got.dtype == np.float32 and np.isfinite(got).all()
    v = T.compare(got, res)
    WORST[c.id] = v.worst
    print("%s: %s" % (c.id, T.describe(v)))
    assert v.outside == 0 and v.nonzero == 0, "%s: %s" % (c.id, T.describe(v))


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_zero_top_and_linearity(m3d, c):
    res = T.reference_of(c)
    zero = backward(m3d, c, np.zeros_like(T.top(c)))
    assert not zero.any()
    g1 = backward(m3d, c, T.top(c))
    g2 = backward(m3d, c, T.top(c) * np.float32(2))
    # |g2 - 2 ref| <= bound(2 top) = 2 bound(top) and |2 g1 - 2 ref| <= 2 bound(top)
    bd = 4.0 * T.bound(res)
    err = np.abs(g2.astype(np.float64) - 2.0 * g1.astype(np.float64))
    where = np.unravel_index(int(np.argmax(err - bd)), err.shape)
    assert (err <= bd).all(), "%s: %d elements; err %g bound %g at %s" % (c.id, (err > bd).sum(), err[where], bd[where], where)
    assert not g2[res.A == 0].any()


def upstream(shape, seed):
    """A seeded upstream gradient of small integers times a power of two per channel.  torch's pool backward then is exact in fp32 and in
    fp64 alike (a sum of at most 8 such numbers, for the average pool divided by 8), so the grad_output the Function received on the GPU
    IS the one computed below on the CPU."""
    rs = np.random.RandomState(seed)
    return (rs.randint(-8, 9, shape) * 2.0 ** rs.randint(-3, 4, (1, shape[1], 1, 1, 1))).astype(np.float32)


@pytest.mark.parametrize("cid", ["avg_wrapper", "shipped"])
@pytest.mark.parametrize("kind", ["plain", "avg", "max"])
def test_autograd_wrappers(m3d, cid, kind):
    from m3d import compat
    c = T.BY_ID[cid]
    B, Cc, S, H, W = c.shape
    rs = np.random.RandomState(3000 + T.CASES.index(c))
    feat = dev((rs.randn(*c.shape) * np.exp(rs.randn(1, Cc, 1, 1, 1))).astype(np.float32)).requires_grad_()
    rois = dev(T.rois(c)).requires_grad_()
    mod = {"plain": compat.RoIAlign_3d, "avg": compat.RoIAlignAvg_3d, "max": compat.RoIAlignMax_3d}[kind](7, 7, 7, c.scale, 2)
    out = mod(feat, rois)
    assert out.shape == (c.R, Cc, 7, 7, 7)
    up = upstream(tuple(out.shape), 4000 + T.CASES.index(c))
    upd = dev(up)
    if kind == "plain":                       # the same values behind permuted strides: the Function has to make them contiguous
        upd = upd.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
        assert not upd.is_contiguous() and torch.equal(upd, dev(up))
    out.backward(upd)
    assert rois.grad is None and feat.grad is not None and feat.grad.shape == feat.shape

    if kind == "plain":
        bins, go = (7, 7, 7), up.astype(np.float64)
    else:
        # the Function's forward output (a deterministic kernel: the module's result is its pool, bit for bit), pooled on the CPU in fp64
        bins = (8, 8, 8)
        pool = F.avg_pool3d if kind == "avg" else F.max_pool3d
        with torch.no_grad():
            y = mod._fn(1)(feat.detach(), rois.detach())
            assert y.shape == (c.R, Cc, 8, 8, 8) and torch.equal(pool(y, kernel_size=2, stride=1), out)
        y64 = y.cpu().double().requires_grad_()
        pool(y64, kernel_size=2, stride=1).backward(torch.from_numpy(up).double())
        go = y64.grad.numpy()
        assert np.array_equal(go.astype(np.float32).astype(np.float64), go)
    res = T.reference(go, T.rois(c), c.shape, bins, c.scale, 2)
    assert (res.A > 0).any()
    v = T.compare(feat.grad.cpu().numpy(), res)
    print("%s through %s: %s" % (cid, type(mod).__name__, T.describe(v)))
    assert v.outside == 0 and v.nonzero == 0, "%s through %s: %s" % (cid, type(mod).__name__, T.describe(v))


def test_refused_configuration_raises_and_writes_nothing(m3d):
    from m3d._lib import lib
    q = T.REFUSED
    B, Cc, S, H, W = q["shape"]
    AS, AH, AW = q["bins"]
    rois = dev(q["rois"])
    top = torch.ones((rois.shape[0], Cc, AS, AH, AW), device="cuda")
    with pytest.raises(m3d.M3DError):
        m3d.roi_align3d_backward(top, rois, q["shape"], AS, AH, AW, q["scale"], q["ratio"])
    grad = torch.full(q["shape"], 7.25, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib().m3d_roi_align3d_backward(AS, AH, AW, C.c_float(q["scale"]), q["ratio"], C.c_void_p(top.data_ptr()), C.c_void_p(rois.data_ptr()),
                                        rois.shape[0], 7, C.c_void_p(grad.data_ptr()), B, Cc, S, H, W, stream)
    torch.cuda.synchronize()
    assert rc == T.M3D_EUNSUPPORTED
    assert bool((grad == 7.25).all())
    # the same call one ratio lower is taken and does write
    rc = lib().m3d_roi_align3d_backward(AS, AH, AW, C.c_float(q["scale"]), 9, C.c_void_p(top.data_ptr()), C.c_void_p(rois.data_ptr()),
                                        rois.shape[0], 7, C.c_void_p(grad.data_ptr()), B, Cc, S, H, W, stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((grad != 7.25).any())
