"""CPU: the case table of tests/conv_f16_narrow_cases.py against the library's host queries (m3d_conv3d_zn_supported,
m3d_conv3d_zn_packed_bytes, m3d_conv3d_zn_launch_units), the contract on the exact emulation of the cut (integers exact; every random
family within E; every seeded defect leaves E and breaks the integer exactness - the tests can fail), and the routing
(conv_plan.plan_conv / train_conv_kernel with the new arguments, m3d.compat.set_conv_train_narrow)."""
import ctypes as C
import itertools
import types

import pytest
import torch

import conv_f16_narrow_cases as T


def check(got, y, E):
    """True when got meets E everywhere"""
    return bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


@pytest.fixture(scope="module")
def L():
    from m3d._lib import lib
    return lib()


# ------------------------------------------------------------------ the table against the library
def test_every_case_is_supported_and_the_refusals(L):
    for name, (B, cin, cout, D, H, W) in T.CASES.items():
        assert L.m3d_conv3d_zn_supported(cin, cout, D, H, W) == 1, name
        assert W <= 8 and cin % 16 == 0
    assert L.m3d_conv3d_zn_supported(32, 64, 7, 7, 9) == 0
    assert L.m3d_conv3d_zn_supported(8, 64, 7, 7, 7) == 0
    assert L.m3d_conv3d_zn_supported(24, 64, 7, 7, 7) == 0
    assert L.m3d_conv3d_zn_supported(32, 64, 0, 7, 7) == 0 and L.m3d_conv3d_zn_supported(32, 0, 7, 7, 7) == 0


def test_packed_bytes_is_a_function_of_the_channels(L):
    seen = {}
    for B, cin, cout, D, H, W in T.CASES.values():
        n = int(L.m3d_conv3d_zn_packed_bytes(cin, cout))
        assert n > 0 and n % 16 == 0
        assert seen.setdefault((cin, cout), n) == n
        # [cout group 64][chunk x 27 taps][block 2][hi / lo][k half][row 32] 16-byte units + the 256-byte tail that holds max|w|
        assert n == ((cout + 63) // 64) * (cin // 16) * 27 * 256 * 16 + 256
    assert L.m3d_conv3d_zn_packed_bytes(24, 64) == 0 and L.m3d_conv3d_zn_packed_bytes(0, 64) == 0


def test_launch_units_and_the_ragged_walk_condition(L):
    for name, (B, cin, cout, D, H, W) in T.CASES.items():
        units = int(L.m3d_conv3d_zn_launch_units(B, cin, cout, D, H, W))
        assert units == B * ((cout + 63) // 64) * ((H + 7) // 8) * ((D + 3) // 4), name
    B, cin, cout, D, H, W = T.CASES["ragged_walk"]
    units = int(L.m3d_conv3d_zn_launch_units(B, cin, cout, D, H, W))
    assert (cin, D, H, W) == (16, 7, 7, 7) and units > T.CUS and units % T.CUS != 0 and units < 2 * T.CUS
    assert int(L.m3d_conv3d_zn_launch_units(1, *T.CASES["cout5"][1:])) == 1


def test_null_pointers_are_refused_before_they_are_followed(L):
    BAD = C.c_void_p(64)
    assert L.m3d_conv3d_zn_pack(None, 32, 16, BAD, None) == -1 and L.m3d_conv3d_zn_pack(BAD, 32, 16, None, None) == -1
    assert L.m3d_conv3d_zn_pack(BAD, 24, 16, BAD, None) == -1
    assert L.m3d_conv3d_zn_pack_dgrad(None, 32, 16, BAD, None) == -1 and L.m3d_conv3d_zn_pack_dgrad(BAD, 32, 24, BAD, None) == -1
    assert L.m3d_conv3d_zn_forward(None, BAD, BAD, 1, 32, 16, 7, 7, 7, None, None, 0, BAD, None, None) == -1
    assert L.m3d_conv3d_zn_forward(BAD, BAD, BAD, 1, 32, 16, 7, 7, 9, None, None, 0, BAD, None, None) == -4
    assert L.m3d_conv3d_zn_forward(BAD, BAD, BAD, 1, 24, 16, 7, 7, 7, None, None, 0, BAD, None, None) == -4


# ------------------------------------------------------------------ integers
@pytest.mark.parametrize("case", sorted(T.CASES))
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_integer_operands_are_exact_and_every_geometry_defect_breaks_that(direction, case):
    """the cut of a small integer is exact (l = 0) and the sums stay below 2^24: the emulation EQUALS the fp64 reference
    (conv_f16_narrow_cases.integer_inputs)"""
    a, wl, shift = T.integer_inputs(case, direction)
    want = T.reference_op(direction, a, wl, None, shift)
    assert torch.equal(T.emulated(a, wl, shift=shift), want)
    _, al = T.cut(a, float(a.abs().max()))
    assert bool((al == 0).all())
    assert float(T.terms(T.conv3d_op, a, wl)[0].max()) < 2.0 ** 24
    for d in T.GEOMETRY_DEFECTS:
        assert not torch.equal(T.emulated(a, wl, shift=shift, defect=d), want), d


# ------------------------------------------------------------------ random families
@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("case", sorted(T.CASES))
def test_the_cut_meets_the_bound_and_every_seeded_defect_leaves_it(case, family):
    for direction in T.DIRECTIONS:
        a, wl, scale, shift, relu, y, E, Cm = T.reference(case, direction, family)
        assert check(T.emulated(a, wl, scale, shift, relu), y, E), direction
        if direction == "dgrad":          # the launched conv on the flipped, transposed weight IS the transposed conv
            assert torch.allclose(T.finish(T.conv3d_op(a.double(), wl.double())), y, rtol=1e-9, atol=1e-12 * float(y.abs().max()) + 1e-300)
            continue                      # (the defects below: once per case and family, on the forward form with its epilogue)
        loose = 4.0 * float(a.abs().max())                                  # a deliberately loose bound: E from that A
        yl, El, _ = T.contract(direction, a, wl, scale, shift, relu, in_bound=loose)
        assert check(T.emulated(a, wl, scale, shift, relu, in_bound=loose), yl, El)
        for m in T.CUT_MUTANTS:
            assert not check(T.emulated(a, wl, scale, shift, relu, mutant=m), y, E), m
        if family == "at_bound_below":    # one exponent too high: the largest operand overflows fp16
            assert not check(T.emulated(a, wl, scale, shift, relu, mutant="scale_up"), y, E)
        for d in T.GEOMETRY_DEFECTS:
            if d == "halo_z" and a.shape[2] == 1 and family.startswith("at_bound"):
                continue                  # does not apply: on one plane the shift only swaps the tap plane, and these weights are constant
            assert not check(T.emulated(a, wl, scale, shift, relu, defect=d), y, E), d


# ------------------------------------------------------------------ routing
def _layer(cin, cout, k=3, pool=False, narrow=True):
    """a LayerConv's planning face without packs: the library's host queries only"""
    from m3d import ops
    zw = zn = None
    if k == 3 and cin % 16 == 0:
        zw = ops.ZwConv3d.__new__(ops.ZwConv3d)
        zw.cin, zw.cout = cin, cout
        if narrow and not pool:
            zn = ops.ZnConv3d.__new__(ops.ZnConv3d)
            zn.cin, zn.cout = cin, cout
    conv = ops.PackedConv3d.__new__(ops.PackedConv3d)
    conv.k, conv.cin, conv.cout = k, cin, cout
    return types.SimpleNamespace(cin=cin, cout=cout, k=k, pool=pool, stem=None, wino=None, zw=zw, zn=zn, conv=conv)


BODY = [(32, 64, True), (64, 64, False), (64, 128, True), (128, 128, False), (128, 256, True), (256, 256, False), (256, 256, False)]
HEADS = [(256, 128), (128, 128), (256, 256), (32, 32)]


def _grid():
    """(batch, cin, cout, pool, D, H, W): the body's layers on their maps, the head shapes on 7^3 and 14^3, the case table"""
    out = []
    for (cin, cout, pool), n in itertools.product(BODY, (64, 32, 16, 8)):
        out += [(b, cin, cout, pool, n, n, n) for b in (1, 4)]
    for (cin, cout), n, R in itertools.product(HEADS, (7, 14), (1, 16, 31, 32, 64, 128, 1000)):
        out.append((R, cin, cout, False, n, n, n))
    out += [(B, cin, cout, False, D, H, W) for B, cin, cout, D, H, W in T.CASES.values()]
    out += [(64, 32, 64, False, 7, 7, 9), (64, 32, 64, False, 7, 7, 11), (64, 24, 64, False, 7, 7, 7), (64, 32, 24, False, 7, 7, 7)]
    return out


def test_plan_conv_moves_only_the_narrow_maps(L):
    from m3d import conv_plan as P
    moved = 0
    for B, cin, cout, pool, D, H, W in _grid():
        layer = _layer(cin, cout, pool=pool)
        shape = (B, D, H, W)
        base = P.plan_conv(layer, shape)
        assert P.plan_conv(layer, shape, narrow_f16=False) == base
        assert P.plan_conv(_layer(cin, cout, pool=pool, narrow=False), shape, narrow_f16=True) == base      # no narrow pack: nothing moves
        on = P.plan_conv(layer, shape, narrow_f16=True)
        want = (not pool and W <= 8 and cin % 16 == 0 and not L.m3d_conv3d_zw_supported(cin, cout, D, H, W, 0)
                and L.m3d_conv3d_zn_launch_units(B, cin, cout, D, H, W) >= P.ZN_MIN_UNITS)
        assert on == (P.Plan(P.ZN, False, True) if want else base), (B, cin, cout, pool, D, H, W)
        moved += want
    assert moved > 0 and P.plan_conv(_layer(256, 128), (128, 7, 7, 7), narrow_f16=True).kind == P.ZN
    assert P.plan_conv(_layer(256, 128), (128, 14, 14, 14), narrow_f16=True).kind != P.ZN               # ZwConv3d takes the 14^3 maps


def test_train_conv_kernel_moves_only_the_narrow_maps(L):
    from m3d import conv_plan as P
    for (B, cin, cout, pool, D, H, W), mode, direction in itertools.product(_grid(), ("fp32", "f16x2"), ("forward", "dgrad")):
        base = P.train_conv_kernel(direction, B, cin, cout, D, H, W, mode)
        assert P.train_conv_kernel(direction, B, cin, cout, D, H, W, mode, narrow=False) == base
        on = P.train_conv_kernel(direction, B, cin, cout, D, H, W, mode, narrow=True)
        ci, co = (cin, cout) if direction == "forward" else (cout, cin)
        want = (W <= 8 and ci % 16 == 0 and L.m3d_conv3d_zn_launch_units(B, ci, co, D, H, W) >= P.ZN_MIN_UNITS)
        assert on == (P.TRAIN_F16X2_NARROW if want else base), (direction, mode, B, cin, cout, D, H, W)
        assert base != P.TRAIN_F16X2_NARROW
    assert P.train_conv_kernel("forward", 128, 256, 128, 7, 7, 7, "fp32", k=1, narrow=True) == P.TRAIN_FP32
    # dgrad swaps the roles: a forward layer 24 -> 32 launches a 32 -> 24 conv
    assert P.train_conv_kernel("dgrad", 128, 24, 32, 7, 7, 7, "fp32", narrow=True) == P.TRAIN_F16X2_NARROW
    assert P.train_conv_kernel("forward", 128, 24, 32, 7, 7, 7, "fp32", narrow=True) == P.TRAIN_FP32


def test_the_switch_round_trips_and_install_leaves_it_off():
    import m3d
    import m3d.compat as c
    assert m3d.ZnConv3d is m3d.ops.ZnConv3d
    assert c.get_conv_train_narrow() is False
    assert c.set_conv_train_narrow(True) is False and c.get_conv_train_narrow() is True
    assert c.get_conv_train() == "fp32"                                     # independent of set_conv_train
    assert c.set_conv_train_narrow(False) is True and c.get_conv_train_narrow() is False
    c.install()
    try:
        assert c.get_conv_train_narrow() is False
    finally:
        c.uninstall_conv3d()
        c.uninstall_linear()


def test_dgrad_of_and_supported_refuse_what_the_library_refuses():
    from m3d import ops
    Z = ops.ZnConv3d
    assert Z.supported(torch.empty(64, 32, 3, 3, 3)) and Z.supported(torch.empty(5, 16, 3, 3, 3), (2, 8, 8))
    assert not Z.supported(torch.empty(64, 24, 3, 3, 3)) and not Z.supported(torch.empty(64, 32, 3, 3, 3), (7, 7, 9))
    assert not Z.supported(torch.empty(64, 32, 1, 1, 1))
    for shape in ((24, 32, 3, 3, 3), (32, 32, 1, 1, 1), (32, 32, 3, 3)):
        with pytest.raises(ValueError):
            Z.dgrad_of(torch.empty(shape))
