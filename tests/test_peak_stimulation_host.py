"""CPU: the NumPy restatement of the peak stimulation contract (tests/peak_stimulation_reference.py) against the recorded results of
the reference's own function (tests/golden/peak_stimulation.npz, written by tests/golden/gen_peak_stimulation.py) and against
torch-CPU's max_pool3d formulation (lib/prm/peak_stimulation_3d.py:15-25); and every refusal of the three C entry points, which are made
before a device pointer is followed and therefore need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import peak_stimulation_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "peak_stimulation.npz")
EINVAL, EUNSUPPORTED = -1, -4


def golden_cases():
    z = np.load(GOLDEN)
    return z, [str(n) for n in z["names"]]


def case_filter(z, name):
    """The restatement's `filt` argument of a recorded case."""
    kind = str(z[name + "_filter"])
    if kind == "none":
        return None
    if kind == "const":
        return float(z[name + "_value"])
    if kind == "tensor":
        return z[name + "_thresh"]
    return kind


def test_golden_covers_the_cases():
    z, names = golden_cases()
    assert os.path.getsize(GOLDEN) < 200 * 1024
    kinds = {str(z[n + "_filter"]) for n in names}
    assert kinds == {"none", "median", "mean", "max", "const", "tensor"}
    assert {int(z[n + "_win"]) for n in names} == {1, 3, 5}
    assert any(np.isnan(z[n + "_x"]).sum() == 2 for n in names)
    assert any(z[n + "_peaks"].shape[0] == 0 and np.isnan(z[n + "_agg"]).all() for n in names)
    med = [int(np.prod(z[n + "_x"].shape[2:])) % 2 for n in names if str(z[n + "_filter"]) == "median"]
    assert 0 in med and 1 in med


@pytest.mark.parametrize("name", golden_cases()[1])
def test_restatement_equals_golden(name):
    z, _ = golden_cases()
    x = z[name + "_x"]
    got = R.peak_stimulation(x, int(z[name + "_win"]), case_filter(z, name))
    assert np.array_equal(got["peaks"], z[name + "_peaks"])
    assert np.array_equal(got["thresh"], z[name + "_thresh"], equal_nan=True)
    assert np.array_equal(got["agg"], z[name + "_agg"], equal_nan=True)          # NaN positions included
    assert np.array_equal(R.backward(got["peak_map"], z[name + "_gy"]), z[name + "_gx"], equal_nan=True)


def torch_formulation(x, win):
    """peak_stimulation_3d.py:14-25 restated on torch-CPU: -inf padding, max_pool3d with indices, indices == arange."""
    o = win // 2
    t = torch.from_numpy(x)
    p = F.pad(t, (o,) * 6, value=float("-inf"))
    s, h, w = p.shape[2:]
    el = torch.arange(s * h * w).view(1, 1, s, h, w)
    if o:
        el = el[:, :, o:-o, o:-o, o:-o]
    _, ind = F.max_pool3d(p, kernel_size=win, stride=1, return_indices=True)
    return (ind == el).numpy()


def test_restatement_equals_torch_maxpool_formulation():
    rng = np.random.RandomState(7)
    for case in range(20):
        shape = (int(rng.randint(1, 3)), int(rng.randint(1, 4))) + tuple(int(v) for v in rng.randint(1, 9, 3))
        win = int(rng.choice([1, 3, 5, 7, 9]))
        levels = int(rng.choice([2, 3, 5, 17]))
        x = (rng.randint(0, levels, shape) / 4.0 - 1.0).astype(np.float32)              # tied values, both signs, zeros
        if case % 4 == 3 and x.size > 4:
            x.reshape(-1)[rng.choice(x.size, 2, replace=False)] = np.nan
        if case % 5 == 4:
            x[x == 0] = -0.0
        assert np.array_equal(R.local_maxima(x, win), torch_formulation(x, win)), (case, shape, win)


def test_restatement_thresholds_equal_torch():
    rng = np.random.RandomState(11)
    for n_sp in ((3, 5, 7), (2, 4, 4)):                                                  # odd and even n
        x = (rng.randint(-8, 9, (2, 3) + n_sp) / 8.0).astype(np.float32)
        x[0, 0, 0, 0, 0] = -0.0
        x[1, 2, 1, 1, 1] = np.nan
        t = torch.from_numpy(x).reshape(2, 3, -1)
        assert np.array_equal(R.thresholds(x, "median"), t.median(2)[0].numpy(), equal_nan=True)
        assert np.array_equal(R.thresholds(x, "max"), t.max(2)[0].numpy(), equal_nan=True)
        assert np.array_equal(R.thresholds(x, "mean"), t.mean(2).numpy(), equal_nan=True)   # multiples of 1/8: exact either way


# ------------------------------------------------------------------------------------------------ refusals of the C entry points
@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


FAKE = C.c_void_p(4096)          # a non-NULL "device pointer" that a refusing call never follows


def fwd(L, B=1, Cn=1, S=4, H=4, W=4, win=3, kind=0, x=FAKE, thr_in=None, peaks=FAKE, cap=8, num=FAKE, thresh=FAKE, ws=FAKE, ws_bytes=0):
    return L.m3d_peak_stimulation3d(x, B, Cn, S, H, W, win, kind, C.c_float(0.0), thr_in, None, peaks, cap, num, None, thresh, None, ws,
                                    C.c_size_t(ws_bytes), None)


def test_refusals_without_gpu(L):
    big = 1 << 40
    for win in (0, -1, -3, 2, 4, 10):
        assert fwd(L, win=win, ws_bytes=big) == EINVAL, win
    for win in (11, 13, 101):
        assert fwd(L, win=win, ws_bytes=big) == EUNSUPPORTED, win
    for kind in (-1, 6, 99):
        assert fwd(L, kind=kind, ws_bytes=big) == EINVAL, kind
    for dims in (dict(S=0), dict(H=0), dict(W=0), dict(S=-1), dict(B=-1), dict(Cn=-2)):
        assert fwd(L, ws_bytes=big, **dims) == EINVAL, dims
    for null in ("x", "num", "thresh", "ws", "peaks"):
        assert fwd(L, ws_bytes=big, **{null: None}) == EINVAL, null
    assert fwd(L, kind=5, thr_in=None, ws_bytes=big) == EINVAL                           # TENSOR without d_thresh_in
    assert fwd(L, cap=-1, ws_bytes=big) == EINVAL
    need = L.m3d_peak_stimulation3d_workspace_bytes(1, 1, 4, 4, 4, 3)
    assert need > 0
    assert fwd(L, ws_bytes=need - 1) == EINVAL                                           # workspace too small
    assert fwd(L, ws_bytes=0) == EINVAL
    assert fwd(L, S=2048, H=1024, W=1024, ws_bytes=big) == EUNSUPPORTED                  # S H W = 2^31
    assert fwd(L, S=1 << 11, H=1 << 10, W=(1 << 10) - 1, win=4, ws_bytes=big) == EINVAL
    # empty B * C: nothing is done, whatever the pointers are
    assert fwd(L, B=0, x=None, thresh=None, ws=None) == 0
    assert fwd(L, Cn=0, x=None, thresh=None, ws=None) == 0


def test_workspace_bytes(L):
    f = L.m3d_peak_stimulation3d_workspace_bytes
    assert f(1, 1, 4, 4, 4, 2) == 0 and f(1, 1, 4, 4, 4, 11) == 0 and f(1, 1, 0, 4, 4, 3) == 0 and f(0, 3, 4, 4, 4, 3) == 0
    assert f(1, 1, 2048, 1024, 1024, 3) == 0
    a, b = f(1, 35, 16, 16, 16, 3), f(2, 35, 16, 16, 16, 3)
    assert 35 * 4096 <= a < b                                                            # holds at least the byte map


def test_backward_refusals_without_gpu(L):
    g = L.m3d_peak_stimulation3d_backward
    assert g(None, FAKE, 1, 1, 4, 4, 4, FAKE, None) == EINVAL
    assert g(FAKE, None, 1, 1, 4, 4, 4, FAKE, None) == EINVAL
    assert g(FAKE, FAKE, 1, 1, 4, 4, 4, None, None) == EINVAL
    assert g(FAKE, FAKE, 1, 1, 0, 4, 4, FAKE, None) == EINVAL
    assert g(FAKE, FAKE, -1, 1, 4, 4, 4, FAKE, None) == EINVAL
    assert g(FAKE, FAKE, 1, 1, 2048, 1024, 1024, FAKE, None) == EUNSUPPORTED
    assert g(None, None, 0, 4, 4, 4, 4, None, None) == 0


def test_op_refuses_cpu_tensors(L):
    import m3d
    with pytest.raises(m3d.M3DError):
        m3d.peak_stimulation_3d(torch.zeros((1, 1, 4, 4, 4)))
    with pytest.raises(m3d.M3DError):
        m3d.peak_stimulation_3d_dev(torch.zeros((1, 1, 4, 4, 4)))
