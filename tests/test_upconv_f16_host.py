"""CPU: the accuracy contract of the up-conv's f16x2 forward and of the fused mask-head tail (tests/upconv_f16_cases.py) - the emulated cut
lies within E_u on every case and family, each wrong cut breaks E_u on a named (case, family), the fp64 references agree with
tests/upconv_reference.py - and the library's host-only answers: _supported, _packed_bytes, and every refusal before a pointer is followed."""
import ctypes as C

import numpy as np
import pytest
import torch

import upconv_f16_cases as T
import upconv_reference as UR

EINVAL, EUNSUPPORTED, OK = -1, -4, 0


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("case", sorted(T.CASES) + sorted(T.EXTRA_CASES))
def test_the_emulated_cut_lies_within_E_u(case, family):
    x, w, bu, _, _, y, Eu, C_, _, _ = T.reference(case, family)
    got = T.emulated(x, w, bu, relu=True)
    r = T.worst(got, y, Eu)
    assert r <= 1.0, "%s %s: emulated cut at %.3g of E_u" % (case, family, r)
    bias_only = torch.relu(bu.to(T.F64)).view(1, -1, 1, 1, 1).expand_as(y)
    assert torch.equal(got[C_ == 0], bias_only[C_ == 0])                # no products: exactly the bias path


@pytest.mark.parametrize("mutant", T.CUT_MUTANTS)
def test_each_wrong_cut_breaks_E_u(mutant):
    case, family = T.MUTANT_SITES[mutant]
    x, w, bu, _, _, y, Eu, _, _, _ = T.reference(case, family)
    r = T.worst(T.emulated(x, w, bu, relu=True, mutant=mutant), y, Eu)
    assert r > 1.0, "%s on %s %s stays at %.3g of E_u: the bound cannot see it" % (mutant, case, family, r)


@pytest.mark.parametrize("case", ("one", "ragged", "roi_grid", "wide_row"))
def test_fp64_references_agree_with_upconv_reference(case):
    x, w, bu, wc, bc, y, _, C_, l, _ = T.reference(case, "benign")
    y_np, A_np = UR.forward(x.numpy(), w.numpy(), bu.numpy(), relu=True)
    assert np.abs(y.numpy() - y_np).max() <= 1e-12 * max(1.0, float(np.abs(y_np).max()))
    assert np.abs(C_.numpy() + np.abs(bu.double().numpy())[None, :, None, None, None] - A_np).max() <= 1e-12 * float(A_np.max())
    l_np = np.einsum("kc,rcdhw->rkdhw", wc.double().numpy(), y_np) + bc.double().numpy()[None, :, None, None, None]
    assert np.abs(l.numpy() - l_np).max() <= 1e-12 * max(1.0, float(np.abs(l_np).max()))


@pytest.mark.parametrize("defect", T.GEOMETRY_DEFECTS)
def test_each_geometry_defect_misses_E_l(defect):
    x, w, bu, wc, bc, _, _, _, l, El = T.reference("roi_grid", "benign")
    assert T.worst(T.defective_logits(x, w, bu, wc, bc, defect), l, El) > 1.0


@pytest.fixture(scope="module")
def L():
    from m3d._lib import lib
    return lib()


def test_supported_and_packed_bytes(L):
    for R, cin, cout, D, H, W, K in T.CASES.values():
        assert L.m3d_upconv3d_2x_f16x2_supported(R, cin, cout, D, H, W) == 1
        # [32-channel block][k step][8 parities][hi / lo][64 lanes] 16-byte units + 256 bytes for fl(max|W|)
        assert L.m3d_upconv3d_2x_f16x2_packed_bytes(cin, cout) == (cout + 31) // 32 * (cin // 16) * 8 * 2 * 64 * 16 + 256
    assert L.m3d_upconv3d_2x_f16x2_supported(0, 16, 1, 1, 1, 1) == 1          # an empty batch is a supported shape
    assert L.m3d_upconv3d_2x_f16x2_supported(1, 1040, 3, 1, 2, 3) == 1       # more channels than one staged chunk
    for bad in ((1, 8, 4, 2, 2, 2), (1, 24, 4, 2, 2, 2), (1, 0, 4, 2, 2, 2), (1, 16, 0, 2, 2, 2), (1, 16, 4, 0, 2, 2), (-1, 16, 4, 2, 2, 2),
                (1 << 20, 16, 4, 8, 8, 8),             # x: 2^33 elements
                (1 << 14, 16, 64, 8, 8, 8),            # x fits (2^27), y = 2^14 64 8 512 = 2^32 does not
                (1, 1 << 15, 1 << 14, 1, 1, 1)):       # the weight: 2^32 elements
        assert L.m3d_upconv3d_2x_f16x2_supported(*bad) == 0, bad
    assert L.m3d_upconv3d_2x_f16x2_packed_bytes(24, 4) == 0 and L.m3d_upconv3d_2x_f16x2_packed_bytes(16, 0) == 0


def test_refusals_come_before_any_pointer_is_followed(L):
    p = C.c_void_p(4096)                                # never followed: every call below returns before a launch
    odd, p8 = C.c_void_p(4098), C.c_void_p(4104)

    def plain(x=p, pk=p, b=p, y=p, R=2, cin=32, cout=8, D=2, H=2, W=2, im=p):
        return L.m3d_upconv3d_2x_forward_f16x2(x, pk, b, y, R, cin, cout, D, H, W, 1, im, None)

    def tail(x=p, pk=p, b=p, wc=p, bc=p, o=p, R=2, cin=32, cout=8, K=2, D=2, H=2, W=2, im=p):
        return L.m3d_mask_tail_f16x2(x, pk, b, wc, bc, o, R, cin, cout, K, D, H, W, 1, im, None)

    for f in (plain, tail):
        assert f(R=0, x=None, pk=None, im=None) == OK                           # an empty batch: nothing is looked at
        assert f(R=-1) == EINVAL and f(cin=0) == EINVAL and f(cout=0) == EINVAL and f(D=0) == EINVAL
        assert f(cin=24) == EUNSUPPORTED and f(cin=8) == EUNSUPPORTED
        assert f(R=1 << 20, D=8, H=8, W=8) == EUNSUPPORTED
        assert f(x=None) == EINVAL and f(pk=None) == EINVAL and f(im=None) == EINVAL
        assert f(x=odd) == EINVAL and f(b=odd) == EINVAL
        assert f(pk=p8) == EUNSUPPORTED
    assert plain(y=None) == EINVAL and plain(y=C.c_void_p(4100)) == EUNSUPPORTED
    assert tail(o=None) == EINVAL and tail(wc=None) == EINVAL and tail(o=C.c_void_p(4100)) == EUNSUPPORTED
    assert tail(K=0) == EUNSUPPORTED and tail(K=9) == EUNSUPPORTED and tail(K=-1) == EUNSUPPORTED
    assert L.m3d_upconv3d_2x_f16x2_pack(p, 24, 4, p, None) == EUNSUPPORTED
    assert L.m3d_upconv3d_2x_f16x2_pack(None, 16, 4, p, None) == EINVAL and L.m3d_upconv3d_2x_f16x2_pack(p, 16, 4, None, None) == EINVAL
    assert L.m3d_upconv3d_2x_f16x2_pack(p, 0, 4, p, None) == EINVAL and L.m3d_upconv3d_2x_f16x2_pack(p, 16, 4, p8, None) == EUNSUPPORTED
