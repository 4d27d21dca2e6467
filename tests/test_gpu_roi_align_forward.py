"""GPU: every fp32 path of the RoIAlign3D forward (csrc/roi_align3d.hip) against the fp64 reference of tests/roi_align_forward_cases.py,
element by element, with its derived bound |got - ref| <= (n_o + 4) * 2^-24 * A_o.  Which code path computes which RoI of the table,
and that the table reaches every path under every hand-over kind, is proved on the CPU by tests/test_roi_align_forward_cases_host.py.

 (a) every case through the four C entry points (m3d_roi_align3d_forward, _forward_ws with a workspace = heavy-first launch order,
     _forward_ws with a null workspace, _forward_exact) into a buffer the test owns, pre-filled with 7.25 and again with NaN: every element
     inside the bound, exactly 0.0 where no sample is valid, no sentinel and no NaN left - every element is written on every route and
     hand-over kind; the exact entry equals the oracle bit for bit, the ordered launch equals the index-order launch bit for bit;
 (b) two calls on fresh buffers are bit-equal (no atomics in the forward);
 (c) class markers a previous call could have left in a recycled output buffer change nothing;
 (d) m3d_roi_align3d_tap_tables equals the host tables exactly;
 (e) ops.roi_align3d_forward (default, exact=True) and compat's RoIAlign Function and module meet the same bound;
 (f) the tuning build's XCD-aware channel split (tune_roi_xcd = 1) gives the bits of the default split."""
import ctypes as C

import numpy as np
import pytest
import torch

import roi_align_forward_cases as Fc

pytestmark = pytest.mark.gpu

ENTRIES = ("forward", "ws", "ws_null", "exact")
WORST = {}
_DEV = {}


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    yield _m
    _DEV.clear()
    for cid, r in WORST.items():
        print("RoIAlign3D forward: largest |got - ref| / bound  %-18s %s" % (cid, "  ".join("%s %.4f" % kv for kv in sorted(r.items()))))


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the table's arrays are read-only


def operands(c):
    if c.id not in _DEV:
        _DEV[c.id] = (dev(Fc.features(c)), dev(Fc.rois(c)))
    return _DEV[c.id]


def vp(t):
    return C.c_void_p(t.data_ptr())


def c_call(c, entry, fill, prefill=None):
    """one C entry point into a [R, C, AS, AH, AW] buffer filled with `fill` (and then treated by `prefill`): the buffer"""
    from m3d._lib import lib
    L = lib()
    B, Cc, S, H, W = c.shape
    f, r = operands(c)
    out = torch.full((c.R, Cc) + c.bins, fill, dtype=torch.float32, device="cuda")
    if prefill is not None:
        prefill(out)
    head = (c.bins[0], c.bins[1], c.bins[2], C.c_float(c.scale), c.ratio, vp(f), B, Cc, S, H, W, vp(r), c.R, 7, vp(out))
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry == "forward":
        rc = L.m3d_roi_align3d_forward(*head, stream)
    elif entry == "exact":
        rc = L.m3d_roi_align3d_forward_exact(*head, stream)
    elif entry == "ws":
        wsb = int(L.m3d_roi_align3d_workspace_bytes(c.R))
        assert wsb > 0
        ws = torch.full((wsb,), 255, dtype=torch.uint8, device="cuda")
        rc = L.m3d_roi_align3d_forward_ws(*head, vp(ws), C.c_size_t(wsb), stream)
    else:
        rc = L.m3d_roi_align3d_forward_ws(*head, None, C.c_size_t(0), stream)
    torch.cuda.synchronize()
    assert rc == 0, (c.id, entry, rc)
    return out


def within(c, got, what):
    """assert the bound on a device tensor in the output's memory order; returns the verdict"""
    v = Fc.compare(got.cpu().numpy(), Fc.reference_of(c))
    print("%s, %s: %s" % (c.id, what, Fc.describe(v)))
    assert v.outside == 0 and v.nonzero == 0, "%s, %s: %s" % (c.id, what, Fc.describe(v))
    return v


@pytest.mark.parametrize("fill", [7.25, float("nan")], ids=["sentinel", "nan"])
@pytest.mark.parametrize("c", Fc.CASES, ids=Fc.case_id)
def test_every_entry_point_against_fp64(m3d, c, fill):
    outs = {}
    for entry in ENTRIES:
        out = outs[entry] = c_call(c, entry, fill)
        got = out.cpu().numpy()
        # (a computed 7.25 would be counted as unwritten; none of the table's references is 7.25, and the NaN run is the unambiguous one)
        left = int(np.isnan(got).sum() + (got == 7.25).sum())
        assert left == 0, "%s, %s: %d elements were not written" % (c.id, entry, left)
        v = within(c, out, entry)
        w = WORST.setdefault(c.id, {})
        w[entry] = max(w.get(entry, 0.0), v.worst)
    assert np.array_equal(outs["exact"].cpu().numpy(), Fc.oracle_of(c))               # the reference's operation order: bit-exact
    assert torch.equal(outs["ws"], outs["ws_null"])                                    # heavy-first order: the same rows, the same bits
    assert torch.equal(outs["forward"], outs["ws_null"])


@pytest.mark.parametrize("c", Fc.CASES, ids=Fc.case_id)
def test_two_calls_are_bit_equal(m3d, c):
    for entry in ("ws", "forward"):
        a, b = c_call(c, entry, 7.25), c_call(c, entry, float("nan"))
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)


@pytest.mark.parametrize("kind", list(Fc.MARKERS) + ["mixed"])
def test_stale_class_markers_change_nothing(m3d, kind):
    """A recycled output buffer may hold the markers of the call before it - the kernel's own bit patterns at exactly the places the
    kernels read them (element 0 of every 8th channel), e.g. every RoI marked `small`.  roi_class_kernel rewrites every one of them first."""
    c = Fc.BY_ID["marks_c64"]
    assert all(rt.handover == "marks" for rt in Fc.routes_of(c))
    bits = np.array(list(Fc.MARKERS.values()), np.uint32).view(np.int32)

    def prefill(out):
        flat = out.view(torch.int32).view(c.R, c.shape[1], -1)
        if kind == "mixed":
            rs = np.random.RandomState(7)
            flat[:, ::8, 0] = dev(bits[rs.randint(0, len(bits), (c.R, c.shape[1] // 8))])
        else:
            flat[:, ::8, 0] = int(np.uint32(Fc.MARKERS[kind]).view(np.int32))
        assert int(torch.isnan(out).sum()) == c.R * c.shape[1] // 8

    for entry in ("ws", "ws_null"):
        clean = c_call(c, entry, 0.0)
        assert torch.equal(c_call(c, entry, 0.0, prefill), clean)
        within(c, clean, entry)


@pytest.mark.parametrize("c", Fc.V3_CASES, ids=Fc.case_id)
def test_tap_tables_equal_the_host_tables(m3d, c):
    from m3d._lib import lib
    B, _, S, H, W = c.shape
    _, r = operands(c)
    tab = torch.full((c.R, 3, 14, 4), -7, dtype=torch.int32, device="cuda")
    batch = torch.full((c.R,), -7, dtype=torch.int32, device="cuda")
    rc = lib().m3d_roi_align3d_tap_tables(vp(r), c.R, C.c_float(c.scale), B, S, H, W, vp(tab), vp(batch),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    want = [Fc.tap_table(row, c.scale, (S, H, W), B) for row in Fc.rois(c)]
    got = tab.cpu().numpy()
    for i, (t, b) in enumerate(want):
        assert np.array_equal(got[i], t), (c.id, i, got[i], t)       # lo, hi and the BITS of h * valid, l * valid
    assert np.array_equal(batch.cpu().numpy(), np.array([b for _, b in want], np.int32))
    assert (got[..., 2:] != 0).any() and (got[..., 2] == 0).any()    # valid and invalid samples both occur


@pytest.mark.parametrize("cid", [Fc.SHIPPED, "adaptive_222", "noncubic"])
def test_wrappers_meet_the_bound(m3d, cid):
    from m3d import compat
    c = Fc.BY_ID[cid]
    f, r = operands(c)
    args = (f, r, c.bins[0], c.bins[1], c.bins[2], c.scale, c.ratio)
    fast = m3d.roi_align3d_forward(*args)
    assert fast.shape == (c.R, c.shape[1]) + c.bins
    within(c, fast, "ops.roi_align3d_forward")
    within(c, m3d.roi_align3d_forward(*args, ordered=False), "ops.roi_align3d_forward(ordered=False)")
    exact = m3d.roi_align3d_forward(*args, exact=True)
    within(c, exact, "ops.roi_align3d_forward(exact=True)")
    assert np.array_equal(exact.cpu().numpy(), Fc.oracle_of(c))
    fn = compat.RoIAlignFunction_3d(c.bins[0], c.bins[1], c.bins[2], c.scale, c.ratio)
    within(c, fn(f, r), "compat.RoIAlignFunction_3d")
    mod = compat.RoIAlign_3d(c.bins[0], c.bins[1], c.bins[2], c.scale, c.ratio)
    out = mod(f.clone().requires_grad_(), r)
    assert out.requires_grad
    within(c, out.detach(), "compat.RoIAlign_3d")
    assert torch.equal(out.detach(), fast)


def test_xcd_channel_split_of_the_tuning_build(m3d):
    """tune_roi_xcd = 1 (tuning build only; C a multiple of 64 and the markers' hand-over): another split of the same channels over
    workgroups, the same arithmetic per row"""
    from m3d import _lib
    c = Fc.BY_ID["marks_c64"]
    assert c.shape[1] % 64 == 0
    with _lib.tuning():
        if not _lib.lib().m3d_tuning_build():
            pytest.skip("release build: no mutable options, tune_roi_xcd cannot be set")
        prev = _lib.get_option("tune_roi_xcd")
        try:
            _lib.set_option("tune_roi_xcd", 0)
            base = {e: c_call(c, e, float("nan")) for e in ("ws", "ws_null")}
            _lib.set_option("tune_roi_xcd", 1)
            assert _lib.get_option("tune_roi_xcd") == 1
            for e in ("ws", "ws_null"):
                got = c_call(c, e, float("nan"))
                assert torch.equal(got, base[e])
                within(c, got, "tune_roi_xcd = 1, " + e)
        finally:
            _lib.set_option("tune_roi_xcd", prev)
