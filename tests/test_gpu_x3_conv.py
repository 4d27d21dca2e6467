"""The bf16x3 / f16x2 direct conv of csrc/conv3d_x3.hip (ops.X3Conv3d, the norm conv of the peak back-propagation) against fp64, element by
element, on the case table of tests/x3_conv_cases.py (tests/test_x3_conv_cases_host.py proves what the table reaches and that this
module's comparisons catch every seeded defect):
  integers   every element EQUALS the fp64 reference, through ops.X3Conv3d and through the C entry points on NaN-filled `out` and workspace
             with guard rows behind both (every element written, none accumulated onto stale memory, nothing stored past cout); the
             split launch equals the unsplit one bit for bit
  random     every element within the derived bound of x3_conv_cases.bound, exactly 0 where sum |a| |w| == 0 and nowhere else; the f16x2
             form with the exact and the 2^8-loose in_max; a second call is bit-identical
The worst |got - y| / bound per (form, ksplit) is printed at the end of the module (pytest -s); the module docstring of x3_conv_cases.py
records the figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import x3_conv_cases as T

pytestmark = pytest.mark.gpu

WORST = {}
_convs = {}


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    for (form, ksplit), r in sorted(WORST.items()):
        print("x3 conv: worst |got - y| / bound  %-3s ksplit %d  %.4f" % (form, ksplit, r))
    _convs.clear()
    torch.cuda.empty_cache()


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()


def conv_of(ops, c, w, tag):
    """the packed weights, once per (form, mode, shape, operand family)"""
    key = (c._replace(ws=True, ksplit=0), tag)
    if key not in _convs:
        _convs[key] = ops.X3Conv3d(dev(w), c.mode, f16=(c.form == "x3f"))
    return _convs[key]


def scalars(c, x, off, loose=False):
    """(in_offset, in_max) as the device scalars the launch reads"""
    offd = None if off is None else torch.tensor([off], dtype=torch.float32, device="cuda")
    maxd = torch.tensor([T.in_max_of(c, x, off, loose)], dtype=torch.float32, device="cuda") if c.form == "x3f" else None
    return offd, maxd


def same(c, got, ref, what, ksplit):
    """bit-equal to the fp64 reference cast to fp32; on a mismatch, where the wrong elements lie: voxel tiles, cout tiles, 32-row blocks and
    the position inside the 16 x 4 tile name the path, NaN counts tell a missed store from a wrong sum"""
    got = torch.as_tensor(got).reshape(ref.shape)
    ref = ref.to(torch.float32)
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    b, co, z, y, x = (bad[:, i] for i in range(5))
    tiles = sorted(set(zip((x // T.TX).tolist(), (y // T.TY).tolist(), (z // T.TZ).tolist())))
    raise AssertionError(
        "%s %s (ksplit %d, K ranges %s): %d of %d elements differ (%d NaN); first (b, c, z, y, x) %s got %r want %r; last %s; items %s; "
        "cout tiles %s; 32-row blocks %s; (x, y, z) tiles %s; x %% 16 %s; y %% 4 %s; z %% 4 %s"
        % (T.case_id(c), what, ksplit, T.k_ranges(c, ksplit), bad.shape[0], ref.numel(), int(torch.isnan(got).sum()), bad[0].tolist(),
           float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]), bad[-1].tolist(), sorted(set(b.tolist())),
           sorted(set((co // T.TM).tolist())), sorted(set((co % T.TM // 32).tolist())), tiles[:12], sorted(set((x % T.TX).tolist())),
           sorted(set((y % T.TY).tolist())), sorted(set((z % T.TZ).tolist()))))


def run_entry(ops, c, conv, xd, offd, maxd, use_ws):
    """one launch through the C entry points on NaN memory -> (Buffers of host arrays, ksplit of the launch): `out` is followed by
    GUARD_ROWS channel maps of SENTINEL, and so is the workspace; use_ws False: m3d_conv3d_x3_forward (f16x2: a null workspace)"""
    L = ops.lib()
    dims = (c.batch, c.cin, c.cout, c.D, c.H, c.W)
    n, guard = T.elems(c), T.GUARD_ROWS * c.D * c.H * c.W
    buf = torch.full((n + guard,), float("nan"), dtype=torch.float32, device="cuda")
    buf[n:] = T.SENTINEL
    wsb = int(L.m3d_conv3d_x3_workspace_bytes(*dims)) if use_ws else 0
    ws = None
    if wsb:
        ws = torch.full((wsb // 4 + guard,), float("nan"), dtype=torch.float32, device="cuda")
        ws[wsb // 4:] = T.SENTINEL
    P, st = ops._ptr, ops._stream()
    if c.form == "x3f":
        rc = L.m3d_conv3d_x3f_forward_ws(P(xd), P(conv.packed), P(buf), *dims, P(offd), P(maxd), P(ws), C.c_size_t(wsb), st)
    elif use_ws:
        rc = L.m3d_conv3d_x3_forward_ws(P(xd), P(conv.packed), P(buf), *dims, P(offd), P(ws), C.c_size_t(wsb), st)
    else:
        rc = L.m3d_conv3d_x3_forward(P(xd), P(conv.packed), P(buf), *dims, P(offd), st)
    ops.check(rc, "conv3d_x3 entry point")
    torch.cuda.synchronize()
    return T.Buffers(buf.cpu().numpy(), None if ws is None else ws[wsb // 4:].cpu().numpy()), (wsb // (4 * n) or 1)


def check_buffers(c, got, y, what, ksplit):
    want = T.expected(c, y.numpy(), ksplit)
    same(c, got.out[:T.elems(c)], y, what, ksplit)
    assert np.array_equal(got.out[T.elems(c):], want.out[T.elems(c):]), "%s %s: the guard rows behind `out` were written" % (T.case_id(c), what)
    assert (got.ws_guard is None) == (want.ws_guard is None), (T.case_id(c), what, ksplit)
    assert got.ws_guard is None or np.array_equal(got.ws_guard, want.ws_guard), "%s %s: the guard rows behind the workspace were written" % (
        T.case_id(c), what)
    assert T.same_buffers(got, want)


# ------------------------------------------------------------------ integers: exact
@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_exact_on_integers_through_the_op(ops, c):
    x, w, off = T.integer_operands(c)
    y, _ = T.integer_reference(c)
    conv = conv_of(ops, c, w, "int")
    by_ws, by_units = T.queried_ksplit(ops.lib(), c)
    assert by_ws == by_units == conv.workgroups((c.batch, c.cin, c.D, c.H, c.W)) // T.units(c) and (by_ws == c.ksplit or not c.ws)
    xd = dev(x)
    for loose in ((False, True) if c.form == "x3f" else (False,)):
        offd, maxd = scalars(c, x, off, loose)
        got = conv(xd, in_offset=offd, in_max=maxd)
        same(c, got.cpu(), y, "X3Conv3d%s" % (" loose in_max" if loose else ""), by_ws)


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_exact_on_integers_through_the_entry_points_on_nan_memory(ops, c):
    """`out` and the workspace start as NaN: an element nothing stored, or a first flush that adds to what memory holds, stays NaN; the
    guard rows behind both keep their sentinel; and the launch that splits K equals the one that does not, bit for bit"""
    x, w, off = T.integer_operands(c)
    y, _ = T.integer_reference(c)
    conv = conv_of(ops, c, w, "int")
    xd = dev(x)
    offd, maxd = scalars(c, x, off)
    got, ksplit = run_entry(ops, c, conv, xd, offd, maxd, c.ws)
    assert ksplit == c.ksplit, (T.case_id(c), ksplit)
    check_buffers(c, got, y, "entry point", ksplit)
    if c.ksplit > 1:
        whole, one = run_entry(ops, c, conv, xd, offd, maxd, False)
        assert one == 1
        check_buffers(c, whole, y, "entry point without a workspace", 1)
        assert np.array_equal(whole.out, got.out)


# ------------------------------------------------------------------ random data: within the bound
@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_random_data_is_within_the_bound_at_every_element(ops, c):
    x, w, off = T.random_operands(c)
    conv = conv_of(ops, c, w, "rnd")
    xd = dev(x)
    for loose in ((False, True) if c.form == "x3f" else (False,)):
        offd, maxd = scalars(c, x, off, loose)
        y, E, S = T.bound(c, x, w, off, T.in_max_of(c, x, off, loose) if c.form == "x3f" else None)
        first, ksplit = run_entry(ops, c, conv, xd, offd, maxd, c.ws)
        assert ksplit == c.ksplit
        again, _ = run_entry(ops, c, conv, xd, offd, maxd, c.ws)
        assert np.array_equal(first.out, again.out), "%s: a second call differs from the first" % T.case_id(c)
        assert np.array_equal(first.out[T.elems(c):], T.expected(c, y.numpy()).out[T.elems(c):])
        got = torch.from_numpy(first.out[:T.elems(c)].astype(np.float64)).reshape(y.shape)
        assert bool(torch.isfinite(got).all()), T.case_id(c)
        err = (got - y).abs()
        ratio = float((err / E.clamp_min(1e-300)).max())
        at = np.unravel_index(int((err / E.clamp_min(1e-300)).argmax()), tuple(y.shape))
        print("x3 conv %s%s: worst |got - y| / bound %.4f at %s (y %.3e)" % (T.case_id(c), " loose" if loose else "", ratio, at, float(y[at])))
        key = (c.form, c.ksplit)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        zero = S == 0
        assert bool(zero.any()) and bool((got[zero] == 0).all()), T.case_id(c)
        assert torch.equal(got == 0, zero), T.case_id(c)      # (f16x2: no output of these operands has every product below the cut's floor)
        assert ratio <= 1.0, (T.case_id(c), loose, ratio, at)
