"""Operand bounds of the f16x2 box-head GEMMs that travel with the activations instead of being swept: the feature maps' bound from
the slots the last conv's epilogue filled, fc2's from the launch that stores fc1's output (split-K reduce, or the GEMM's own epilogue
when K is not split) - each bit-equal to the sweep it replaces, and the GEMM outputs with them bit-equal to those with the swept bound."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    yield _m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("side", [32, 128])
def test_conv_body_leaves_max_abs_in_its_slots(m3d, side):
    """Every layer output that carries bound slots: their largest entry == the sweep of that output, bit for bit.  At 32^3 the deeper
    maps (8^3, 4^3) are below what the f16x2 conv takes (12 voxels per side and a minimum of work units, m3d/conv_plan.py), so the feature
    maps themselves carry no slots and the box head sweeps them, as for any tensor from elsewhere; on the 4 x 128^3 batch of a detection
    step (16^3 maps) conv4b's epilogue leaves them."""
    from m3d.config import Cfg
    from m3d.model import DetectorM3D
    from m3d.synth import make_params
    P = make_params(stride=8, num_anchors=5, mlp_dim=64, seed=1)
    det = DetectorM3D({k: v.cuda() for k, v in P.items()}, Cfg.nuclei(mlp_dim=64))
    assert det.conv_f16
    vol = torch.randn((1 if side == 32 else 4, 1, side, side, side), generator=torch.Generator().manual_seed(2)).cuda()
    carried = []
    for last in range(1, len(det.body) + 1):
        y = det.conv_body(vol, last=last)
        slots = det._carried_bound(y)
        carried.append(slots is not None)
        if slots is not None:
            assert slots.numel() == m3d.ZwConv3d.SLOTS
            assert torch.equal(slots.max().view(1), m3d.ops.absmax(y)), last
        assert float(y._m3d_head_bound.abs().max()) == 0.0 and y._m3d_head_bound.numel() == m3d.ZwConv3d.SLOTS
    assert any(carried) and (carried[-1] or side < 128)


# (rows, N, K): K = 64 is not split (slices == 1: the GEMM's epilogue stores and bounds), the others are (the reduce does);
# 130 / 70 rows: a ragged last row tile; 400 x 256: the 256 x 256 tiles
SHAPES = [(130, 128, 64), (130, 128, 10976), (70, 64, 2048), (400, 256, 64), (400, 256, 4096)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("relu", [True, False])
def test_slot_bounds_in_and_out(m3d, M, N, K, relu):
    ops = m3d.ops
    g = torch.Generator().manual_seed(M + K)
    w, b = (torch.randn(N, K, generator=g) / K ** 0.5).cuda(), torch.randn(N, generator=g).cuda()
    x = (torch.randn(M, K, generator=g) * 3).cuda()
    lin = ops.SplitLinearF16(w, b)
    split = int(m3d._lib.lib().m3d_linear_f16x2_workspace_bytes(M, N, K)) > 256
    assert split == (K > 64)
    one = ops.absmax(x)
    want = lin(x, relu=relu, x_bound=one)
    slots = torch.zeros((ops.ZwConv3d.SLOTS,), device="cuda")
    slots[5], slots[31] = one[0], one[0] * 0.25
    out_b = torch.zeros((ops.ZwConv3d.SLOTS,), device="cuda")
    got = lin(x, relu=relu, x_bound=slots, out_bound=out_b)
    assert torch.equal(got, want)                                        # the largest slot is the bound: the same scale, the same bits
    assert torch.equal(out_b.max().view(1), ops.absmax(want))            # what the sweep in front of the next layer would find
    # ... and the next layer with it
    lin2 = ops.SplitLinearF16((torch.randn(64, N, generator=g) / N ** 0.5).cuda(), None)
    assert torch.equal(lin2(got, relu=True, x_bound=out_b), lin2(got, relu=True))


def test_roi_align_gemm_form_takes_slot_bounds(m3d):
    """RoIAlign3D's matrix-core form (small sub-volumes): the scale from the largest slot == the scale from the swept maximum"""
    ops = m3d.ops
    g = torch.Generator().manual_seed(4)
    feat = torch.randn((2, 32, 4, 6, 6), generator=g).cuda()
    lo = torch.rand((40, 3), generator=g) * 20
    rois = torch.cat([torch.randint(0, 2, (40, 1), generator=g).float(), lo, lo + 4 + torch.rand((40, 3), generator=g) * 10], 1).cuda()
    one = ops.absmax(feat)
    slots = torch.zeros((ops.ZwConv3d.SLOTS,), device="cuda")
    slots[3], slots[30] = 0.125 * one[0], one[0]
    want = ops.roi_align3d_forward(feat, rois, 7, 7, 7, 0.125, 2, feat_absmax=one)
    assert torch.equal(ops.roi_align3d_forward(feat, rois, 7, 7, 7, 0.125, 2, feat_absmax=slots), want)
