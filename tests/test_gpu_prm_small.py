"""GPU: both small-window GEMMs of the peak back-propagation - m3d_prm_small_dgrad_f16 (csrc/prm_small_f16.hip, the default of
ops.SmallWindowDgrad) and m3d_prm_small_dgrad (csrc/prm_small.hip) - element by element against fp64 over the tables of
tests/prm_small_cases.py (what the tables reach, that the operands are exact and that the comparison catches seeded defects is proved on
the CPU by tests/test_prm_small_cases_host.py).  Per kernel: exact operands and lo-plane probes bit for bit, run-to-run and sub-batch
equality, every input family within the derived per-element bound with exact zeros where nothing is summed, the scale clamp's edge,
the raw C entry points and the pack entry points between guard bands, the launch cap and the workspace check.  The worst
|got - y| / bound per kernel and window size is printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import f16x2_contract as K
import prm_small_cases as S
import prm_stage_cases as T

pytestmark = pytest.mark.gpu

F32 = np.float32
KINDS = ("f16", "f32")
WORST = {}
GUARD = 300                                                             # floats on both sides of a guarded buffer
EWORKSPACE, EUNSUPPORTED = -3, -4


def kid(v):
    return v if isinstance(v, str) else S.case_id(v) if isinstance(v, S.SmallCase) else str(v)


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    for site, r in sorted(WORST.items()):
        print("prm small: worst |got - y| / bound  %-22s %.4f" % (site, r))
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a device error (a fault in a kernel under test) ends the run: nothing more is launched on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error, no further launches: %s" % e, returncode=3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scalar(v):
    return torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def note(site, what, r):
    WORST[site] = max(WORST.get(site, 0.0), r)
    print("prm small ratio: %-16s %-44s %.4f" % (site, what, r))
    assert r <= 1.0, (site, what, r)


def make_op(ops, kind, w):
    op = ops.SmallWindowDgrad(dev(w)) if kind == "f16" else ops.SmallWindowDgrad(dev(w), f16=False)
    assert op.f16 == (kind == "f16")
    return op


def run(ops, kind, e, op=None):
    op = op or make_op(ops, kind, e["w"])
    return op(dev(e["gn"]), dev(e["full"]), scalar(e["off"]), dev(e["origin"])).cpu().numpy()


def bits_equal(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


# ------------------------------------------------------------------ exact comparison, run to run
@pytest.mark.parametrize("kind,c", [(k, c) for k in KINDS for c in S.CASES[k]], ids=kid)
def test_exact(ops, kind, c):
    e, y, ca = S.exact_reference(kind, c)
    assert (ca / (2.0 ** e["kp"]).reshape(-1, 1, 1, 1, 1)).max() < S.LIMIT
    op = make_op(ops, kind, e["w"])
    got = run(ops, kind, e, op)
    T.same_bits(got, y, "%s %s" % (kind, S.case_id(c)), sums=True)     # every peak, every channel, every voxel
    assert bits_equal(run(ops, kind, e, op), got), "a second run differs"
    if kind == "f16":                                                   # the fp32 form takes the same operands (any channel count)
        T.same_bits(run(ops, "f32", e), y, "fp32 form on %s" % S.case_id(c), sums=True)


@pytest.mark.parametrize("which", S.PROBES)
@pytest.mark.parametrize("win", [3, 5, 7])
def test_lo_plane_probes(ops, win, which):
    e, y, _ = S.probe_reference(win, which)
    for kind in KINDS:
        got = run(ops, kind, e)
        T.same_bits(got, y, "%s probe %s win %d" % (kind, which, win), sums=True)


# ------------------------------------------------------------------ bounded comparison
@pytest.mark.parametrize("kind,c,family", [(k, c, f) for k in KINDS for c, f in S.bounded_table(k)], ids=kid)
def test_bounded(ops, kind, c, family):
    e, y, b, live = S.bounded_reference(kind, c, family)
    op = make_op(ops, kind, e["w"])
    got = run(ops, kind, e, op)
    assert bits_equal(run(ops, kind, e, op), got), "a second run differs"
    note("%s win %d" % (kind, c.win), S.case_id(c) + " " + family, S.held(got, y, b, live, "%s %s %s" % (kind, S.case_id(c), family)))


def test_clamp_edge(ops):
    """peaks whose largest gradient lies below 2^-111 (the scale clamps at 2^125), next to ordinary ones: E at A_eff = max(A, 2^-111)"""
    e, y, b, live = S.clamp_reference()
    got = run(ops, "f16", e)
    for p in sorted(S.CLAMP_PEAKS):
        r = S.held(got[p:p + 1], y[p:p + 1], b[p:p + 1], live[p:p + 1], "clamp edge peak %d" % p)
        print("prm small ratio: clamp edge, max |G_N| = 2^%d: %.4f" % (S.CLAMP_PEAKS[p], r))
    assert not got[S.CLAMP_ZERO_PEAK].any()
    note("f16 clamp edge", S.case_id(S.CLAMP_CASE), S.held(got, y, b, live, "clamp edge"))


# ------------------------------------------------------------------ a sub-batch computes the batch's rows
@pytest.mark.parametrize("c", [S.SmallCase(3, 48, 33, 24), S.SmallCase(5, 32, 40, 44)], ids=kid)
def test_sub_batch_equals_the_batch_rows(ops, c):
    for exact in (True, False):
        e = S.exact_reference("f16", c)[0] if exact else S.bounded_reference("f16", c, "benign")[0]
        sel = np.arange(c.P)[::2][::-1].copy()                          # every second peak, reversed
        sub = dict(e, gn=e["gn"][sel], origin=e["origin"][sel])
        for kind in KINDS:
            op = make_op(ops, kind, e["w"])
            whole, part = run(ops, kind, e, op), run(ops, kind, sub, op)
            assert bits_equal(part, whole[sel]), (kind, exact)


# ------------------------------------------------------------------ the C entry points between guard bands
def guarded(nfloat, fill):
    """(whole buffer, the 16-byte aligned view of nfloat floats between two GUARD-float bands)"""
    buf = torch.full((nfloat + 2 * GUARD,), fill, dtype=torch.float32, device="cuda")
    view = buf[GUARD:GUARD + nfloat]
    assert view.data_ptr() % 16 == 0
    return buf, view


def bands_untouched(buf, nfloat, fill):
    h = buf.cpu().numpy()
    want = np.full(GUARD, fill, F32)
    return bits_equal(h[:GUARD], want) and bits_equal(h[GUARD + nfloat:], want)


def raw_launch(ops, kind, e, packed, out, ws=None, ws_bytes=None, num_peaks=None):
    """m3d_prm_small_dgrad[_f16] on device buffers; returns the status code"""
    from m3d._lib import lib
    p, L = ops._ptr, lib()
    P, cg, win = e["gn"].shape[:3]
    cx = e["w"].shape[1]
    D, H, W = e["full"].shape[1:]
    t = dict(gn=dev(e["gn"]), full=dev(e["full"]), off=scalar(e["off"]), origin=dev(e["origin"]))
    P = P if num_peaks is None else num_peaks
    if kind == "f16":
        rc = L.m3d_prm_small_dgrad_f16(p(t["gn"]), p(packed), P, cg, cx, win, p(t["full"]), p(t["off"]), p(t["origin"]), D, H, W, p(out),
                                       p(ws), C.c_size_t(ws_bytes), ops._stream())
    else:
        rc = L.m3d_prm_small_dgrad(p(t["gn"]), p(packed), P, cg, cx, win, p(t["full"]), p(t["off"]), p(t["origin"]), D, H, W, p(out),
                                   ops._stream())
    torch.cuda.synchronize()
    return rc


RAW_CASES = {"f16": (S.SmallCase(3, 48, 33, 24), S.SmallCase(5, 32, 40, 44), S.SmallCase(7, 64, 33, 4)),
             "f32": (S.SmallCase(3, 64, 33, 24), S.SmallCase(5, 8, 40, 44), S.SmallCase(7, 256, 64, 2))}


@pytest.mark.parametrize("kind,c", [(k, c) for k in KINDS for c in RAW_CASES[k]], ids=kid)
def test_c_entry_points_between_guard_bands(ops, kind, c):
    from m3d._lib import lib
    L = lib()
    e, y, _ = S.exact_reference(kind, c)
    op = make_op(ops, kind, e["w"])
    want = run(ops, kind, e, op)
    T.same_bits(want, y, "the op", sums=True)
    nout = y.size
    wsb = L.m3d_prm_small_dgrad_f16_workspace_bytes(c.P) if kind == "f16" else 0
    for fill in (float("nan"), -7.0):
        obuf, out = guarded(nout, fill)
        wbuf, ws = guarded(wsb // 4, fill) if kind == "f16" else (None, None)
        assert raw_launch(ops, kind, e, op.packed, out, ws, wsb) == 0
        assert bits_equal(out.cpu().numpy().reshape(y.shape), want), "the C entry point differs from the op (pre-fill %r)" % fill
        assert bands_untouched(obuf, nout, fill), "out's guard bands"
        if kind == "f16":
            assert bands_untouched(wbuf, wsb // 4, fill), "the workspace's guard bands"
            amax = np.abs(e["gn"]).reshape(c.P, -1).max(1)
            assert bits_equal(ws[:c.P].cpu().numpy(), amax), "the per-peak maxima"
            assert bits_equal(ws[c.P:].cpu().numpy(), np.full(wsb // 4 - c.P, fill, F32)), "the workspace behind the maxima"

    # the pack entry point into a NaN-filled buffer: every unit of every plane is written (a NaN operand would reach the output)
    if kind == "f16":
        nbytes = L.m3d_prm_small_dgrad_f16_packed_bytes(c.cg, c.cx)
        pbuf, packed = guarded(nbytes // 4, float("nan"))
        assert L.m3d_prm_small_dgrad_f16_pack(ops._ptr(dev(e["w"])), c.cg, c.cx, ops._ptr(packed), ops._stream()) == 0
    else:
        nbytes = L.m3d_prm_small_dgrad_packed_bytes(c.cg, c.cx)
        pbuf, packed = guarded(nbytes // 4, float("nan"))
        assert L.m3d_prm_small_dgrad_pack(ops._ptr(dev(e["w"])), c.cg, c.cx, ops._ptr(packed), ops._stream()) == 0
    torch.cuda.synchronize()
    assert bands_untouched(pbuf, nbytes // 4, float("nan")), "the packed buffer's guard bands"
    planes = packed[:(nbytes - 256) // 4] if kind == "f16" else packed
    assert bits_equal(planes.cpu().numpy(), op.packed[:planes.numel()].cpu().numpy()), "the packed image"
    assert not torch.isnan(planes).any()                                # (fp16 pairs of finite weights never alias an fp32 NaN pattern here)
    # ... and it is the image the emulation builds from the documented lane order
    if kind == "f16":
        wmax = float(np.maximum(e["w"], 0).max())
        assert float(packed[(nbytes - 256) // 4]) == wmax
        hi, lo = S.pack_image("f16", e["w"])                           # [cb][chunk][tap][lane][j], unscaled
        img = (np.stack([hi, lo], 3) * K.scale_of(wmax)[0]).astype(np.float16)      # [cb][chunk][tap][plane][lane][j]
        got_img = planes.cpu().numpy().view(np.float16)
        assert np.array_equal(got_img.view(np.uint16), img.reshape(-1).view(np.uint16)), "the packed planes against the emulation's"
    else:
        assert bits_equal(planes.cpu().numpy(), S.pack_image("f32", e["w"]).reshape(-1)), "the packed image against the emulation's"
    obuf, out = guarded(nout, float("nan"))
    wbuf, ws = guarded(wsb // 4, float("nan")) if kind == "f16" else (None, None)
    assert raw_launch(ops, kind, e, packed, out, ws, wsb) == 0
    assert bits_equal(out.cpu().numpy().reshape(y.shape), want), "a launch from the freshly packed buffer differs"


def test_launch_cap_and_workspace_check(ops):
    from m3d._lib import lib
    L = lib()
    c = S.SmallCase(3, 48, 33, 24)
    e, y, _ = S.exact_reference("f16", c)
    op = make_op(ops, "f16", e["w"])
    wsb = L.m3d_prm_small_dgrad_f16_workspace_bytes(c.P)
    obuf, out = guarded(y.size, -7.0)
    wbuf, ws = guarded(wsb // 4, -7.0)
    # one peak more than a launch takes: refused before anything is launched (the buffers hold 24 peaks; none may be touched)
    assert raw_launch(ops, "f16", e, op.packed, out, ws, L.m3d_prm_small_dgrad_f16_workspace_bytes(S.F16_MAX_PEAKS + 1),
                      num_peaks=S.F16_MAX_PEAKS + 1) == EUNSUPPORTED
    # a workspace one byte short
    assert raw_launch(ops, "f16", e, op.packed, out, ws, 4 * c.P - 1) == EWORKSPACE
    untouched = np.full(1, -7.0, F32)
    assert bits_equal(obuf.cpu().numpy(), np.broadcast_to(untouched, obuf.shape)), "out was written"
    assert bits_equal(wbuf.cpu().numpy(), np.broadcast_to(untouched, wbuf.shape)), "the workspace was written"
    # exactly enough is taken
    assert raw_launch(ops, "f16", e, op.packed, out, ws, 4 * c.P) == 0
    T.same_bits(out.cpu().numpy().reshape(y.shape), y, "workspace of exactly 4 P bytes", sums=True)
