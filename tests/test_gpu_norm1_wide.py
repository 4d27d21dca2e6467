"""norm1 with 16-byte accesses (csrc/norm1.hip) against NumPy in fp64: sizes around the vector width and around a grid pass, a batch
whose volumes start at every alignment, a base one element off a 16-byte boundary, both input types and both arithmetic modes.
Count and mean are exact (integer sums below 2^53); the variance sum's order is the kernel's: each order is within (n - 1) 2^-53 of the
exact sum (2.3e-10 at n = 2^21), the square root halves it - std within 4.7e-10 relative is the bound the issue sets; the output is the
kernel's own statistics applied in the documented arithmetic, bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 8, 9, 4099, 2 * 4099]
BATCH = 3


def volumes(n, kind):
    g = np.random.RandomState(n)
    v = g.randint(1, 60000, (BATCH, n)).astype(np.uint16)
    if kind == "zeros":
        v[g.rand(BATCH, n) < 0.3] = 0                        # masked-out voxels
        v[:, 0] = 7                                          # (at least one voxel counts in every volume)
    return v


def reference(v, f32_arith, stats):
    mean, std = stats[0], stats[1]
    if f32_arith:
        return (v.astype(np.float32) - np.float32(mean)) / np.float32(std)
    return ((v.astype(np.float64) - mean) / std).astype(np.float32)


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    return _m


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("kind", ["dense", "zeros"])
def test_norm1_against_numpy(m3d, n, dtype, kind):
    v = volumes(n, kind)
    host = v if dtype == "u16" else v.astype(np.float32)
    # one element off a 16-byte boundary: the volumes are a view that starts at element 1 of a larger allocation
    store = torch.zeros((BATCH * n + 9,), dtype=torch.int16 if dtype == "u16" else torch.float32, device="cuda")
    store[1:1 + BATCH * n].copy_(torch.from_numpy(host.view(np.int16) if dtype == "u16" else host).reshape(-1))
    dev = (store.view(torch.uint16) if dtype == "u16" else store)[1:1 + BATCH * n].view(BATCH, n)
    assert dev.data_ptr() % 16 == (2 if dtype == "u16" else 4)
    for f32_arith in (True, False):
        outs = torch.full((BATCH * n + 9,), 123.0, device="cuda")
        out = outs[3:3 + BATCH * n].view(BATCH, n)
        m3d.norm1_batched(dev, f32_arith=f32_arith, out=out)
        assert float(outs[:3].min()) == 123.0 and float(outs[3 + BATCH * n:].min()) == 123.0 == float(outs[3 + BATCH * n:].max())
        for b in range(BATCH):
            got, st = m3d.norm1(dev[b], f32_arith=f32_arith, return_stats=True)
            st = st.cpu().numpy()
            x = v[b].astype(np.float64)
            m = x > 0
            assert st[2] == m.sum() and st[0] == x[m].sum() / m.sum()
            sd = np.sqrt(((x[m] - st[0]) ** 2).sum() / m.sum())
            assert abs(st[1] - sd) <= 4.7e-10 * sd
            with np.errstate(divide="ignore", invalid="ignore"):
                want = reference(v[b], f32_arith, st)
            assert np.array_equal(got.cpu().numpy(), want, equal_nan=True), (b, f32_arith)
            assert np.array_equal(out[b].cpu().numpy(), want, equal_nan=True), (b, f32_arith, "batched")


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_all_zero_volume(m3d, dtype):
    """no voxel counts: 0 / 0 statistics and an all-NaN volume, as before the 16-byte accesses"""
    z = torch.zeros((4099,), dtype=torch.int16 if dtype == "u16" else torch.float32, device="cuda")
    z = z.view(torch.uint16) if dtype == "u16" else z
    for f32_arith in (True, False):
        got, st = m3d.norm1(z, f32_arith=f32_arith, return_stats=True)
        assert float(st[2]) == 0.0 and bool(torch.isnan(st[:2]).all()) and bool(torch.isnan(got).all())
