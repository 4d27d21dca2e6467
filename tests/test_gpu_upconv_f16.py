"""GPU: the up-conv's f16x2 forward and the fused mask-head tail (csrc/upconv3d_f16.hip) through ops.UpConvF16 and the C entry points, on
the cases of tests/upconv_f16_cases.py: every element within E_u / E_l on six input families, small integers bit-equal to fp64, a zero x
exactly the bias path, two runs and a side-stream run bit-identical, the outputs written whole and only there (NaN-sentinel buffer on a
16-byte-aligned, not 64-byte-aligned base), a given bound equal to the swept one, an empty batch, a non-finite operand; fused only: the
three geometry defects miss E_l, and sigmoid = 1 is torch.sigmoid of sigmoid = 0 bit for bit.

Measured on an MI355X (pytest -s prints them), worst |got - ref| / bound per family over the six cases, plain / fused: see DESIGN.md,
"Mask-head tail on the f16 pipe"."""
import ctypes as C

import pytest
import torch

import upconv_f16_cases as T

pytestmark = pytest.mark.gpu
CASES = sorted(T.CASES) + sorted(T.EXTRA_CASES)


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as o
    return o


def dev(*ts):
    return tuple(None if t is None else t.cuda() for t in ts)


def run_both(ops, x, w, bu, wc, bc, in_max=None):
    """(y ReLU'd, logits) of the two epilogues on device operands"""
    up = ops.UpConvF16(w)
    return up(x, in_max, bias=bu, relu=True), up.tail(x, in_max, bu, wc, bc, sigmoid=False)


@pytest.mark.parametrize("case", CASES)
def test_every_element_within_the_bound(ops, case):
    worst_u, worst_l = {}, {}
    for family in T.FAMILIES:
        x, w, bu, wc, bc, y, Eu, C_, l, El = T.reference(case, family)
        gy, gl = run_both(ops, *dev(x, w, bu, wc, bc))
        gy, gl = gy.cpu(), gl.cpu()
        worst_u[family], worst_l[family] = T.worst(gy, y, Eu), T.worst(gl, l, El)
        bias_only = torch.relu(bu).view(1, -1, 1, 1, 1).expand_as(gy)
        assert torch.equal(gy[C_ == 0], bias_only[C_ == 0]), "%s %s: C == 0 is not exactly the bias" % (case, family)
    msg = "%s worst |err| / E per family: plain %s fused %s" % (
        case, " ".join("%s %.3f" % kv for kv in worst_u.items()), " ".join("%s %.3f" % kv for kv in worst_l.items()))
    print(msg)
    assert max(worst_u.values()) <= 1.0 and max(worst_l.values()) <= 1.0, msg


@pytest.mark.parametrize("case", CASES)
def test_integer_operands_are_bit_equal_to_fp64(ops, case):
    x, w, bu, wc, bc = T.integer_inputs(case)
    y = T.finish(T.up_op(x, w), bu, relu=True)
    l = T.classify(y, wc, bc)
    gy, gl = run_both(ops, *dev(x, w, bu, wc, bc))
    assert torch.equal(gy.cpu().double(), y) and torch.equal(gl.cpu().double(), l)
    gy2 = ops.UpConvF16(w.cuda())(x.cuda(), None, bias=None, relu=False)                 # no bias, no ReLU: the bare sum
    assert torch.equal(gy2.cpu().double(), T.up_op(x, w))


@pytest.mark.parametrize("case", CASES)
def test_zero_x_gives_exactly_the_bias_path(ops, case):
    x, w, bu, wc, bc = T.make(case, "benign")
    gy, gl = run_both(ops, *dev(torch.zeros_like(x), w, bu, wc, bc))
    u = torch.relu(bu)
    assert torch.equal(gy.cpu(), u.view(1, -1, 1, 1, 1).expand_as(gy))
    # the classifier on the constant column, in the contract's terms: every voxel holds the same logits, within E_l of fp64
    ref = (wc.double() @ u.double() + bc.double()).view(1, -1, 1, 1, 1)
    E = T.gamma(T.m_fused(w.shape[1])) * ((wc.double().abs() @ u.double()) + bc.double().abs()).view(1, -1, 1, 1, 1)
    g = gl.cpu().double()
    assert bool(((g - ref).abs() <= E).all())
    assert bool((gl == gl[:1, :, :1, :1, :1]).all())


@pytest.mark.parametrize("case", CASES)
def test_runs_are_bit_identical_also_on_a_side_stream(ops, case):
    x, w, bu, wc, bc = dev(*T.make(case, "heavy"))
    a = run_both(ops, x, w, bu, wc, bc)
    b = run_both(ops, x, w, bu, wc, bc)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = run_both(ops, x, w, bu, wc, bc)
    side.synchronize()
    for i in range(2):
        assert torch.equal(a[i], b[i]) and torch.equal(a[i], c[i])


def guarded(n, lead):
    """(whole, view of n floats starting `lead` floats in): NaN everywhere"""
    whole = torch.full((n + lead + 64,), float("nan"), dtype=torch.float32, device="cuda")
    assert whole.data_ptr() % 64 == 0
    return whole, whole[lead:lead + n]


@pytest.mark.parametrize("case", CASES)
def test_outputs_are_written_whole_and_only_there(ops, case):
    R, cin, cout, D, H, W, K = T.CASES.get(case) or T.EXTRA_CASES[case]
    x, w, bu, wc, bc = dev(*T.make(case, "benign"))
    up = ops.UpConvF16(w)
    lead = 68                                           # 272 bytes: 16-byte aligned, not 32- or 64-byte aligned
    wy, y = guarded(R * cout * 8 * D * H * W, lead)
    wl, l = guarded(R * K * 8 * D * H * W, lead)
    assert y.data_ptr() % 16 == 0 and y.data_ptr() % 64 != 0
    up(x, None, bias=bu, relu=True, out=y.view(R, cout, 2 * D, 2 * H, 2 * W))
    up.tail(x, None, bu, wc, bc, sigmoid=True, out=l.view(R, K, 2 * D, 2 * H, 2 * W))
    for whole, mid in ((wy, y), (wl, l)):
        assert not bool(torch.isnan(mid).any()), "an output element was not written"
        assert bool(torch.isnan(whole[:lead]).all()) and bool(torch.isnan(whole[lead + mid.numel():]).all()), "a write outside the output"
    ry, rl = run_both(ops, x, w, bu, wc, bc)
    assert torch.equal(y.view_as(ry), ry) and torch.equal(l.view_as(rl), torch.sigmoid(rl))


@pytest.mark.parametrize("case", ("ragged", "roi_grid"))
def test_a_given_bound_equals_the_swept_one(ops, case):
    x, w, bu, wc, bc = dev(*T.make(case, "outlier8"))
    swept = ops.ZwConv3d.bound_of(x)
    given = torch.zeros_like(swept)
    given[17] = swept.max()                             # any slot may hold the bound
    a = run_both(ops, x, w, bu, wc, bc)
    b = run_both(ops, x, w, bu, wc, bc, in_max=given)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_loose_bound_still_meets_its_own_E(ops):
    x, w, bu, wc, bc, _, _, _, _, _ = T.reference("roi_grid", "benign")
    loose = float(x.abs().max()) * 37.0
    y, Eu, _ = T.contract_up(x, w, bu, True, in_bound=loose)
    l, El = T.contract_fused(x, w, bu, wc, bc, in_bound=loose)
    im = torch.zeros(ops.ZwConv3d.SLOTS, device="cuda")
    im[0] = loose
    gy, gl = run_both(ops, *dev(x, w, bu, wc, bc), in_max=im)
    assert T.worst(gy.cpu(), y, Eu) <= 1.0 and T.worst(gl.cpu(), l, El) <= 1.0


def test_an_empty_batch(ops):
    _, cin, cout, D, H, W, K = T.CASES["ragged"]
    _, w, bu, wc, bc = dev(*T.make("ragged", "benign"))
    up = ops.UpConvF16(w)
    x = torch.empty((0, cin, D, H, W), device="cuda")
    assert tuple(up(x, None, bias=bu, relu=True).shape) == (0, cout, 2 * D, 2 * H, 2 * W)
    assert tuple(up.tail(x, None, bu, wc, bc).shape) == (0, K, 2 * D, 2 * H, 2 * W)
    assert not up.supports((1, cin + 16, D, H, W)) and up.supports((5, cin, D, H, W))


def test_a_non_finite_operand_gives_a_non_finite_result(ops):
    x, w, bu, wc, bc = T.make("roi_grid", "benign")
    for bad in (float("inf"), float("nan")):
        xb = x.clone()
        xb[1, 5, 3, 4, 2] = bad
        gy, gl = run_both(ops, *dev(xb, w, bu, wc, bc))
        # every output of that voxel reads the operand: all eight parities of every channel / class
        assert not bool(torch.isfinite(gy[1, :, 6:8, 8:10, 4:6]).any()) and not bool(torch.isfinite(gl[1, :, 6:8, 8:10, 4:6]).any())


# ------------------------------------------------------------------ fused only
@pytest.mark.parametrize("defect", T.GEOMETRY_DEFECTS)
def test_each_geometry_defect_misses_E_l_where_the_kernel_meets_it(ops, defect):
    x, w, bu, wc, bc, _, _, _, l, El = T.reference("roi_grid", "benign")
    assert T.worst(T.defective_logits(x, w, bu, wc, bc, defect), l, El) > 1.0
    gl = run_both(ops, *dev(x, w, bu, wc, bc))[1]
    assert T.worst(gl.cpu(), l, El) <= 1.0


@pytest.mark.parametrize("case", CASES)
def test_the_fused_sigmoid_is_torch_sigmoid_of_the_logits(ops, case):
    for family in ("benign", "heavy"):
        x, w, bu, wc, bc = dev(*T.make(case, family))
        up = ops.UpConvF16(w)
        logits = up.tail(x, None, bu, wc, bc, sigmoid=False)
        assert torch.equal(up.tail(x, None, bu, wc, bc, sigmoid=True), torch.sigmoid(logits))


def test_the_c_entry_points_match_the_wrapper(ops):
    from m3d._lib import lib, check
    R, cin, cout, D, H, W, K = T.CASES["ragged"]
    x, w, bu, wc, bc = dev(*T.make("ragged", "benign"))
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    packed = torch.empty((L.m3d_upconv3d_2x_f16x2_packed_bytes(cin, cout),), dtype=torch.uint8, device="cuda")
    check(L.m3d_upconv3d_2x_f16x2_pack(p(w), cin, cout, p(packed), st), "pack")
    im = ops.ZwConv3d.bound_of(x)
    y = torch.empty((R, cout, 2 * D, 2 * H, 2 * W), device="cuda")
    o = torch.empty((R, K, 2 * D, 2 * H, 2 * W), device="cuda")
    check(L.m3d_upconv3d_2x_forward_f16x2(p(x), p(packed), p(bu), p(y), R, cin, cout, D, H, W, 1, p(im), st), "forward")
    check(L.m3d_mask_tail_f16x2(p(x), p(packed), p(bu), p(wc), p(bc), p(o), R, cin, cout, K, D, H, W, 0, p(im), st), "tail")
    ry, rl = run_both(ops, x, w, bu, wc, bc)
    assert torch.equal(y, ry) and torch.equal(o, rl)
    assert float(packed[-256:].view(torch.float32)[0]) == float(w.abs().max())        # fl(max|W|) behind the fragments
