"""GPU: the dilation-1 conv weight gradient on maps at most 8 wide (csrc/conv3d_wgrad_narrow.hip, the 2 x 8 x 8 voxel tile) against the
fp64 reference of tests/conv_wgrad_narrow_cases.py:
 (a) exact on integer operands, element by element; twice the same bits;
 (b) within the summation bound on random operands (nothing measured sets it); `pytest -s` prints the worst ratio per case;
 (c) a workspace and a dW pre-filled with NaN give the same bits: every element is written and no stale partial is read;
 (d) a guard band around dW and around the workspace is untouched.
On one MI355X the worst ratio of (b) is 0.018 (the one-tile case; 0.0008 on the 7^3 grid): DESIGN, "Conv box head"."""
import ctypes as C

import pytest
import torch

import conv_wgrad_narrow_cases as T

pytestmark = pytest.mark.gpu


def same(got, ref, what):
    """bit-equal to the fp64 reference cast to fp32; on a mismatch: how many, the first and the last wrong index and the taps that hold one"""
    got, ref = got.cpu(), ref.to(torch.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError("%s: %d of %d elements differ; first %s got %r want %r; last %s; taps (dz, dy, dx) %s"
                             % (what, bad.shape[0], ref.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
                                bad[-1].tolist(), sorted(set(map(tuple, bad[:, 2:].tolist())))))


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_exact_on_integers(case):
    from m3d import ops
    r = T.reference(case, "int")
    x, gy = r["x"].cuda(), r["gy"].cuda()
    got = ops.conv3d_wgrad_narrow(x, gy)
    same(got, r["gw"], "wgrad narrow")
    assert torch.equal(ops.conv3d_wgrad_narrow(x, gy), got)
    assert torch.equal(ops.conv3d_wgrad(x, gy, 3), got)                  # exact operands: the 2 x 4 x 16 kernel gives the same bits
    if case == T.D1_CASE:
        assert (got[:, :, 0] == 0).all() and (got[:, :, 2] == 0).all()


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_bounded_on_random_data(case):
    from m3d import ops
    r = T.reference(case, "randn")
    x, gy = r["x"].cuda(), r["gy"].cuda()
    plan = ops.conv3d_wgrad_narrow_plan(*case)
    assert (plan["tile_x"], plan["tile_y"]) == (8, 8)
    n = T.terms(case) + plan["slots"] + 1
    got = ops.conv3d_wgrad_narrow(x, gy)
    ratio = T.worst_ratio(got.cpu(), r["gw"], r["A"], n)
    print("%s slots %3d: worst |err| / bound %.4f" % (T.case_id(case), plan["slots"], ratio))
    assert ratio < 1.0, ratio
    assert torch.equal(ops.conv3d_wgrad_narrow(x, gy), got)


def _raw_call(x, gy, dw, ws, ws_bytes):
    from m3d import ops
    B, cin, D, H, W = x.shape
    return ops.lib().m3d_conv3d_wgrad_narrow(ops._ptr(x), ops._ptr(gy), ops._ptr(dw), B, cin, gy.shape[1], D, H, W, 3, ops._ptr(ws),
                                             C.c_size_t(ws_bytes), ops._stream())


@pytest.mark.parametrize("case", [T.CASES[3], T.CASES[6]], ids=T.case_id)
def test_every_element_is_written_and_nothing_else(case):
    from m3d import ops
    r = T.reference(case, "randn")
    x, gy = r["x"].cuda(), r["gy"].cuda()
    B, cin, cout, D, H, W = case
    want = ops.conv3d_wgrad_narrow(x, gy)
    wsb = int(ops.lib().m3d_conv3d_wgrad_narrow_workspace_bytes(B, cin, cout, D, H, W, 3))
    assert wsb > 0 and wsb % 4 == 0
    G = 300                                                             # guard floats on each side (no multiple of the 256-byte alignment)
    n = cout * cin * 27
    for fill in (float("nan"), -7.0):
        dbuf = torch.full((G + n + G,), fill, device="cuda")
        wbuf = torch.full((G + wsb // 4 + G,), fill, device="cuda")
        dw, ws = dbuf[G:G + n], wbuf[G:G + wsb // 4]
        assert _raw_call(x, gy, dw, ws, wsb) == 0
        torch.cuda.synchronize()
        assert torch.equal(dw.view(cout, cin, 3, 3, 3), want), "a stale partial or an unwritten element (fill %r)" % fill
        for name, buf, m in (("dW", dbuf, n), ("workspace", wbuf, wsb // 4)):
            for side in (buf[:G], buf[G + m:]):
                ok = torch.isnan(side).all() if fill != fill else (side == fill).all()
                assert bool(ok), "the guard band around %s was written" % name
    # one byte short of the need: refused, nothing written
    dbuf = torch.full((n,), -7.0, device="cuda")
    assert _raw_call(x, gy, dbuf, wbuf, wsb - 1) == -3                  # M3D_EWORKSPACE
    torch.cuda.synchronize()
    assert (dbuf == -7.0).all()


def test_refusals_reach_python():
    from m3d import ops
    from m3d._lib import M3DError
    x, gy = torch.zeros((1, 4, 3, 3, 9)).cuda(), torch.zeros((1, 5, 3, 3, 9)).cuda()
    assert not ops.conv3d_wgrad_narrow_supported(1, 4, 5, 3, 3, 9)
    with pytest.raises(M3DError):
        ops.conv3d_wgrad_narrow(x, gy)
    with pytest.raises(M3DError):
        ops.conv3d_wgrad_narrow_plan(1, 4, 5, 3, 3, 9)
    assert (ops.conv3d_wgrad_narrow(x[..., :8].contiguous(), gy[..., :8].contiguous()) == 0).all()
