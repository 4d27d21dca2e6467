"""The f16x2 contract (tests/f16x2_contract.py) on the CPU: the exact emulation of the cut meets the derived per-element bound E on every
input family, and each plausible bug of the cut (a mutant) breaks E somewhere - the bound is tight enough for the GPU range tests
(test_gpu_f16x2_range.py) to catch such a bug in a kernel."""
import pytest
import torch

import f16x2_contract as K

F64 = torch.float64
FAMILIES = ["benign", "heavy", "outlier12", "outlier24", "outlier36", "quiet", "at_bound_pow2", "at_bound_below"]
CUT_MUTANTS = ["hi_only", "drop_hilo", "lo_unscaled"]


def check(got, y, E):
    """True when got meets E everywhere"""
    return bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


def test_scale_of_is_the_kernels_exponent_arithmetic():
    for j in range(-40, 40):
        s, inv = K.scale_of(2.0 ** j)
        assert s * 2.0 ** j == 2.0 ** 14 and s * inv == 1.0
        bf = K.below(2.0 ** j)
        assert bf < 2.0 ** j and K.scale_of(bf)[0] * bf == 2.0 ** 15 * (1 - 2.0 ** -24)
    assert K.scale_of(0.0)[0] == 2.0 ** 125                      # clamped exponent field (a zero bound)


def test_cut_pieces_reconstruct_within_the_operand_error():
    g = torch.Generator().manual_seed(1)
    a = torch.randn(4096, generator=g) * torch.exp(10 * torch.randn(4096, generator=g))
    A = float(a.abs().max())
    hi, lo = K.cut(a, A)
    e = (a.double() - hi - lo).abs()
    assert bool((e <= 2.0 ** -22 * a.double().abs() + 2.0 ** -39 * A).all())
    assert bool((lo.abs() <= 2.0 ** -11 * a.double().abs() + 2.0 ** -39 * A).all())
    zero = (hi == 0) & (lo == 0)                               # only zeros and operands below A 2^-39 vanish
    assert bool(zero[a == 0].all()) and bool((a[zero].double().abs() <= 2.0 ** -39 * A).all()) and int(zero.sum()) > int((a == 0).sum())


def linear_case(name):
    x, w = K.inputs(name, (24, 96), (20, 96), 7, signed=True, col=True)
    A, B = float(x.abs().max()), float(w.abs().max())
    y = K.linear_op(x.double(), w.double())
    C, Sa, Sb, n = K.terms(K.linear_op, x, w)
    E = K.bound("fc", 96, C, Sa, Sb, n, A, B, y)
    return x, w, A, B, y, E, K.linear_op


def conv_case(name):
    x, w = K.inputs(name, (1, 16, 4, 5, 6), (8, 16, 3, 3, 3), 11, signed=False)
    A, B = float(x.abs().max()), float(w.abs().max())
    y = K.conv3d_op(x.double(), w.double())
    C, Sa, Sb, n = K.terms(K.conv3d_op, x, w)
    E = K.bound("x3f", 16, C, Sa, Sb, n, A, B, y)
    return x, w, A, B, y, E, K.conv3d_op


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("case", [linear_case, conv_case], ids=["linear", "conv"])
def test_gemm_cut_meets_the_bound_and_every_mutant_breaks_it(case, name):
    x, w, A, B, y, E, op = case(name)
    assert check(K.emulate(op, x, w, A, B), y, E)
    loose = K.emulate(op, x, w, A * 2.0 ** 8, B)                 # a bound 2^8 too large: E with that bound still holds
    C, Sa, Sb, n = K.terms(op, x, w)
    El = K.bound("fc" if op is K.linear_op else "x3f", x.shape[1], C, Sa, Sb, n, A * 2.0 ** 8, B, y)
    assert check(loose, y, El)
    for m in CUT_MUTANTS:
        assert not check(K.emulate(op, x, w, A, B, m), y, E), m
    if name == "at_bound_below":
        assert not check(K.emulate(op, x, w, A, B, "scale_up"), y, E)


def zw_case(name):
    x, w = K.inputs(name, (1, 16, 5, 6, 7), (8, 16, 3, 3, 3), 13, signed=True)
    bound = float(x.abs().max())
    y, E, C = K.zw_contract(x, w, bound)
    return x, w, bound, y, E, C


@pytest.mark.parametrize("name", FAMILIES)
def test_zw_cut_meets_the_bound_and_every_mutant_breaks_it(name):
    x, w, bound, y, E, C = zw_case(name)
    assert torch.allclose(K.zw_combine(*K.zw_operands(x.double(), w.double()), x.shape[2]).double(), y, rtol=1e-5,
                          atol=1e-6 * float(y.abs().max()) + 1e-300)         # the decomposition is the conv
    assert check(K.zw_emulate(x, w, bound), y, E)
    yl, El, _ = K.zw_contract(x, w, bound * 2.0 ** 8)
    assert check(K.zw_emulate(x, w, bound * 2.0 ** 8), yl, El)
    for m in CUT_MUTANTS:
        assert not check(K.zw_emulate(x, w, bound, m), y, E), m
    if name == "at_bound_below":
        for m in ("scale_up", "no_v2"):
            assert not check(K.zw_emulate(x, w, bound, m), y, E), m


def test_zw_with_scale_shift_relu_pool_and_all_zero_input():
    g = torch.Generator().manual_seed(3)
    x = torch.relu(torch.randn(1, 16, 4, 6, 8, generator=g)) * 3.0
    w = torch.randn(8, 16, 3, 3, 3, generator=g) * 0.2
    sc, sh = torch.rand(8, generator=g) + 0.5, torch.randn(8, generator=g)
    bound = float(x.abs().max())
    y, E, _ = K.zw_contract(x, w, bound, scale=sc, shift=sh, relu=True, pool=True)
    em = torch.relu(K.zw_emulate(x, w, bound) * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    assert check(torch.nn.functional.max_pool3d(em, 2, 2), y, E)
    hi = torch.relu(K.zw_emulate(x, w, bound, "hi_only") * sc.double().view(1, -1, 1, 1, 1) + sh.double().view(1, -1, 1, 1, 1))
    assert not check(torch.nn.functional.max_pool3d(hi, 2, 2), y, E)
    z = torch.zeros_like(x)
    y0, E0, C0 = K.zw_contract(z, w, 0.0, shift=sh)
    assert bool((C0 == 0).all()) and torch.equal(y0, sh.double().view(1, -1, 1, 1, 1).expand_as(y0))
    assert torch.equal(K.zw_emulate(z, w, 0.0), torch.zeros_like(y0))


def test_roi_reference_is_the_oracles_map_and_the_cut_feature_operand_meets_the_bound():
    """f16x2_contract.roi_align_ref (fp64 sums over the reference kernel's fp32 sample weights) against the oracle's fp32 RoIAlign3D, and
    the contract of the RoI GEMM on the cut feature operand: the emulation meets E, the hi piece alone does not"""
    import oracle as O
    g = torch.Generator().manual_seed(1)
    f = torch.randn(2, 32, 8, 12, 14, generator=g)
    R = 12
    c = torch.rand(R, 3, generator=g) * torch.tensor([14.0, 12.0, 8.0]) * 8
    ext = 8 + 12 * torch.rand(R, 3, generator=g)
    rois = torch.cat([torch.randint(0, 2, (R, 1), generator=g).float(), c - ext / 2, c + ext / 2], 1)
    ref = torch.from_numpy(O.roi_align_3d_forward(f.numpy(), rois.numpy(), 7, 7, 7, 0.125, 2)).double()
    A = float(f.abs().max())
    y, E, C = K.roi_contract(f, rois, 0.125, 2, A)
    assert float((ref - y).abs().max()) <= 1e-6 * A
    fh, fl = K.cut(f, A)
    assert check(K.roi_align_ref(fh + fl, rois, 0.125, 2), y, E)
    assert not check(K.roi_align_ref(fh, rois, 0.125, 2), y, E)
