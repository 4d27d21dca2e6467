"""GPU: the ordered RoIAlign3D backward (csrc/roi_align3d_bwd.hip; DESIGN.md, "RoIAlign3D backward, ordered") against the fp64 reference
of tests/roi_align_backward_cases.py, element by element, with the bound and the extra cases of
tests/roi_align_backward_ordered_cases.py (what the cases reach is proved on the CPU by tests/test_roi_align_backward_ordered_host.py).

 (a) every accepted case and every extra case, through the C call into a buffer pre-filled with 7.25 and again with NaN: every element
     within (n_e + 8) * 2^-24 * A_e, exactly 0.0 where no add lands - so every element was written;
 (b) `adaptive_untabled` raises; the C call leaves the buffer untouched and 1 in the status word;
 (c) two calls are bit-equal; image 0's gradient does not depend on image 1's RoIs; reversed RoIs stay inside the bound;
 (d) top == 0 gives zeros; the gradient of 2 * top is exactly twice the gradient of top;
 (e) RoIAlign_3d / RoIAlignAvg_3d / RoIAlignMax_3d under set_roi_align_backward("ordered"); the default mode still calls the atomic entry;
 (f) one call captured into a graph and replayed twice gives the eager result bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_align_backward_cases as T
import roi_align_backward_ordered_cases as Q

pytestmark = pytest.mark.gpu

ALL = Q.ACCEPTED + Q.EXTRA
WORST = {}


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    yield _m
    for cid, r in WORST.items():
        print("RoIAlign3D backward, ordered: largest |got - ref| / bound  %-18s %.4f" % (cid, r))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the table's arrays are read-only


def ordered(m3d, c, top, rois=None):
    rois = Q.rois(c) if rois is None else rois
    return m3d.roi_align3d_backward_ordered(dev(top), dev(rois), c.shape, c.bins[0], c.bins[1], c.bins[2], c.scale, c.ratio)


def c_call(c, top, rois, fill):
    """m3d_roi_align3d_backward_ordered into a buffer filled with `fill`: (return code, the buffer, the workspace as int32)"""
    from m3d._lib import lib
    B, Cc, S, H, W = c.shape
    R = rois.shape[0]
    grad = torch.full(c.shape, fill, dtype=torch.float32, device="cuda")
    wsb = int(lib().m3d_roi_align3d_backward_ordered_workspace_bytes(R, B))
    ws = torch.full((wsb // 4,), -1, dtype=torch.int32, device="cuda")
    t, r = dev(top), dev(rois)
    rc = lib().m3d_roi_align3d_backward_ordered(c.bins[0], c.bins[1], c.bins[2], C.c_float(c.scale), c.ratio,
                                                C.c_void_p(t.data_ptr() if R else 0), C.c_void_p(r.data_ptr() if R else 0), R, 7,
                                                C.c_void_p(grad.data_ptr()), B, Cc, S, H, W, C.c_void_p(ws.data_ptr()), C.c_size_t(wsb),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, grad, ws


@pytest.mark.parametrize("fill", [7.25, float("nan")], ids=["sentinel", "nan"])
@pytest.mark.parametrize("c", ALL, ids=T.case_id)
def test_kernel_against_fp64(m3d, c, fill):
    res = Q.reference_of(c)
    rc, grad, ws = c_call(c, Q.top(c), Q.rois(c), fill)
    assert rc == 0 and int(ws[0]) == 0
    got = grad.cpu().numpy()
    assert np.isfinite(got).all(), "%s: %d elements were not written" % (c.id, (~np.isfinite(got)).sum())
    v = Q.compare(got, res)
    WORST[c.id] = max(WORST.get(c.id, 0.0), v.worst)
    print("%s: %s" % (c.id, T.describe(v)))
    assert v.outside == 0 and v.nonzero == 0, "%s: %s" % (c.id, T.describe(v))
    assert torch.equal(ordered(m3d, c, Q.top(c)), grad)             # the wrapper (torch.empty) gives the same bits


def test_adaptive_untabled_is_refused_and_writes_nothing(m3d):
    c = T.BY_ID["adaptive_untabled"]
    with pytest.raises(m3d.M3DError):
        ordered(m3d, c, T.top(c))
    rc, grad, ws = c_call(c, T.top(c), T.rois(c), 7.25)
    assert rc == 0 and int(ws[0]) == 1                              # found on the device: the status word, nothing written
    assert bool((grad == 7.25).all())
    rc, grad, ws = c_call(c, T.top(c)[2:], T.rois(c)[2:], 7.25)     # its two tabled RoIs alone are taken
    assert rc == 0 and int(ws[0]) == 0 and bool((grad != 7.25).all())


@pytest.mark.parametrize("cid", ["shipped", "many_rois", "tiled"])
def test_two_calls_are_bit_equal(m3d, cid):
    c = T.BY_ID.get(cid) or Q.EXTRA_BY_ID[cid]
    a = ordered(m3d, c, Q.top(c))
    b = ordered(m3d, c, Q.top(c))
    assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


def test_an_image_does_not_depend_on_the_other_images_rois(m3d):
    c = T.BY_ID["shipped"]
    full = ordered(m3d, c, T.top(c))
    keep = T.rois(c)[:, 0] == 0
    assert keep.any() and (~keep).any() and not keep[:keep.sum()].all()      # image 0's RoIs move up in the list
    part = ordered(m3d, c, T.top(c)[keep], T.rois(c)[keep])
    assert torch.equal(part[0], full[0])
    assert not part[1].any() and full[1].any()


def test_reversed_rois_stay_inside_the_bound(m3d):
    c = T.BY_ID["shipped"]
    got = ordered(m3d, c, T.top(c)[::-1], T.rois(c)[::-1]).cpu().numpy()
    v = Q.compare(got, T.reference_of(c))
    print("shipped, RoIs reversed: %s" % T.describe(v))
    assert v.outside == 0 and v.nonzero == 0, T.describe(v)


@pytest.mark.parametrize("c", ALL, ids=T.case_id)
def test_zero_top_and_exact_doubling(m3d, c):
    assert not ordered(m3d, c, np.zeros_like(Q.top(c))).any()
    g1 = ordered(m3d, c, Q.top(c))
    g2 = ordered(m3d, c, Q.top(c) * np.float32(2))
    assert torch.equal(g2, g1 * 2)                                   # doubling is exact and the order is fixed


def upstream(shape, seed):
    """A seeded upstream gradient of small integers times a power of two per channel (test_gpu_roi_align_backward.py: upstream).  torch's
    pool backward then is exact in fp32 and in fp64 alike, so the grad_output the Function received on the GPU IS the one computed below on
    the CPU."""
    rs = np.random.RandomState(seed)
    return (rs.randint(-8, 9, shape) * 2.0 ** rs.randint(-3, 4, (1, shape[1], 1, 1, 1))).astype(np.float32)


@pytest.mark.parametrize("cid", ["avg_wrapper", "shipped"])
@pytest.mark.parametrize("kind", ["plain", "avg", "max"])
def test_autograd_wrappers_in_ordered_mode(m3d, cid, kind):
    from m3d import compat
    c = T.BY_ID[cid]
    B, Cc, S, H, W = c.shape
    rs = np.random.RandomState(3000 + T.CASES.index(c))
    feat = dev((rs.randn(*c.shape) * np.exp(rs.randn(1, Cc, 1, 1, 1))).astype(np.float32)).requires_grad_()
    rois = dev(T.rois(c)).requires_grad_()
    mod = {"plain": compat.RoIAlign_3d, "avg": compat.RoIAlignAvg_3d, "max": compat.RoIAlignMax_3d}[kind](7, 7, 7, c.scale, 2)
    prev = compat.set_roi_align_backward("ordered")
    try:
        assert prev == "atomic"
        out = mod(feat, rois)
        assert out.shape == (c.R, Cc, 7, 7, 7)
        up = upstream(tuple(out.shape), 4000 + T.CASES.index(c))
        upd = dev(up)
        if kind == "plain":                       # the same values behind permuted strides: the Function has to make them contiguous
            upd = upd.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
            assert not upd.is_contiguous() and torch.equal(upd, dev(up))
        out.backward(upd, retain_graph=True)
        assert rois.grad is None and feat.grad is not None and feat.grad.shape == feat.shape
        first = feat.grad.clone()
        feat.grad = None
        out.backward(upd)
        assert rois.grad is None and torch.equal(feat.grad, first)  # backward twice: the same bits
    finally:
        compat.set_roi_align_backward(prev)
    assert compat.get_roi_align_backward() == "atomic"

    if kind == "plain":
        bins, go = (7, 7, 7), up.astype(np.float64)
    else:
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
    v = Q.compare(first.cpu().numpy(), res)
    print("%s through %s, ordered: %s" % (cid, type(mod).__name__, T.describe(v)))
    assert v.outside == 0 and v.nonzero == 0, "%s through %s: %s" % (cid, type(mod).__name__, T.describe(v))


def test_the_mode_selects_the_entry_point(m3d, monkeypatch):
    from m3d import compat, ops
    c = T.BY_ID["narrow_c"]
    calls = []
    atomic, gather = ops.roi_align3d_backward, ops.roi_align3d_backward_ordered
    monkeypatch.setattr(ops, "roi_align3d_backward", lambda *a: calls.append("atomic") or atomic(*a))
    monkeypatch.setattr(ops, "roi_align3d_backward_ordered", lambda *a: calls.append("ordered") or gather(*a))

    def run():
        feat = torch.randn(c.shape, device="cuda", requires_grad=True)
        compat.RoIAlign_3d(3, 3, 3, c.scale, 2)(feat, dev(T.rois(c))).sum().backward()
        return feat.grad

    assert compat.get_roi_align_backward() == "atomic"
    g0 = run()
    assert calls == ["atomic"]
    prev = compat.set_roi_align_backward("ordered")
    try:
        g1 = run()
        assert calls == ["atomic", "ordered"]
        # an unsupported configuration raises in ordered mode; it does not fall back
        u = T.BY_ID["adaptive_untabled"]
        feat = torch.randn(u.shape, device="cuda", requires_grad=True)
        out = compat.RoIAlign_3d(7, 7, 7, u.scale, 0)(feat, dev(T.rois(u)))
        with pytest.raises(m3d.M3DError):
            out.sum().backward()
        assert calls == ["atomic", "ordered", "ordered"]
    finally:
        compat.set_roi_align_backward(prev)
    assert g0.shape == g1.shape and compat.get_roi_align_backward() == "atomic"


def test_graph_capture(m3d):
    c = T.BY_ID["shipped"]
    top, rois = dev(T.top(c)), dev(T.rois(c))

    def fn():
        return m3d.roi_align3d_backward_ordered(top, rois, c.shape, c.bins[0], c.bins[1], c.bins[2], c.scale, c.ratio)

    eager = fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                    # one stream, two launches in a row: no parallel branches
        out = fn()
    for _ in range(2):
        out.fill_(7.25)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
