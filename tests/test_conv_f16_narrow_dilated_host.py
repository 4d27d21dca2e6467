"""CPU: the dilation-2 narrow-map f16x2 conv (tests/conv_f16_narrow_dilated_cases.py) without a GPU: the case table against the
library's three new host-testable faces (m3d_conv3d_zn_dilated_supported / _launch_units and the refusals of
m3d_conv3d_zn_dilated_forward), the contract on the exact emulation of the cut (integers exact; every case x direction x family within
E), and that the cases can see a wrong kernel: every seeded geometry defect and cut mutant leaves E on at least one case, and on the
RoI grid every one of them does."""
import ctypes as C
import itertools

import pytest
import torch

import conv_f16_narrow_cases as T1
import conv_f16_narrow_dilated_cases as T

EINVAL, EUNSUPPORTED = -1, -4


def check(got, y, E):
    """True when got meets E everywhere"""
    return bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


@pytest.fixture(scope="module")
def L():
    from m3d._lib import lib
    return lib()


# ------------------------------------------------------------------ the table against the library
def test_the_cases_are_the_dilation_1_shapes_and_w2(L):
    cases = T.cases()
    assert tuple(sorted(cases)) == T.CASE_NAMES and len(cases) == len(T1.CASES) + 1
    for name, shape in T1.CASES.items():
        if name != "ragged_walk":
            assert cases[name] == shape
    assert cases["w2"] == (1, 16, 32, 5, 6, 2)
    for name, (B, cin, cout, D, H, W) in cases.items():
        assert L.m3d_conv3d_zn_dilated_supported(cin, cout, D, H, W, 2) == 1, name
    B, cin, cout, D, H, W = cases["ragged_walk"]
    units = int(L.m3d_conv3d_zn_dilated_launch_units(B, cin, cout, D, H, W, 2))
    assert (cin, cout, D, H, W) == (16, 8, 7, 7, 7) and T1.CUS < units < 2 * T1.CUS and units % T1.CUS != 0
    # what the shapes are there for
    assert cases["cout5"][3] == 2 and cases["d1"][3] == 1 and cases["w2"][5] == 2 and cases["w3"][5] == 3
    assert cases["tiles"][3] > 2 * T.TILE_Z + 2 and cases["tiles"][4] > T.TILE_Y + 2


def _shapes():
    out = [(cin, cout, D, H, W) for _, cin, cout, D, H, W in T1.CASES.values()]
    out += [(cin, cout, D, H, W) for cin, cout in ((16, 1), (32, 64), (256, 256), (24, 64), (8, 8), (0, 8), (16, 0), (-16, 8))
            for D, H, W in ((7, 7, 7), (1, 1, 1), (14, 14, 8), (7, 7, 9), (7, 7, 14), (0, 7, 7), (7, 0, 7), (7, 7, 0))]
    out.append((1 << 20, 8, 8, 8, 8))                      # cin D H W = 2^29: the 32-bit offset limit
    return out


def test_supported_and_launch_units_at_dilation_1_are_the_old_queries(L):
    for cin, cout, D, H, W in _shapes():
        old = L.m3d_conv3d_zn_supported(cin, cout, D, H, W)
        assert L.m3d_conv3d_zn_dilated_supported(cin, cout, D, H, W, 1) == old, (cin, cout, D, H, W)
        assert L.m3d_conv3d_zn_dilated_supported(cin, cout, D, H, W, 2) == old, (cin, cout, D, H, W)      # the same limits
        for d in (0, 3, 4, -1):
            assert L.m3d_conv3d_zn_dilated_supported(cin, cout, D, H, W, d) == 0
        for B in (1, 5, 300, 0, -2):
            old_units = int(L.m3d_conv3d_zn_launch_units(B, cin, cout, D, H, W))
            assert int(L.m3d_conv3d_zn_dilated_launch_units(B, cin, cout, D, H, W, 1)) == old_units
            assert int(L.m3d_conv3d_zn_dilated_launch_units(B, cin, cout, D, H, W, 3)) == 0
    for name, (B, cin, cout, D, H, W) in T.cases().items():
        # (64 output channels) x (8 x 8 x 4 voxels): the tile the dilation-2 instantiation was built with
        assert int(L.m3d_conv3d_zn_dilated_launch_units(B, cin, cout, D, H, W, 2)) == B * ((cout + 63) // 64) * ((H + 7) // 8) * ((D + 3) // 4)


def test_refusals_come_before_a_pointer_is_followed(L):
    BAD = C.c_void_p(64)                 # never followed
    fwd = L.m3d_conv3d_zn_dilated_forward

    def call(d_in=BAD, packed=BAD, out=BAD, batch=1, cin=32, cout=16, D=7, H=7, W=7, dil=2, in_max=BAD):
        return fwd(d_in, packed, out, batch, cin, cout, D, H, W, dil, None, None, 0, in_max, None, None)
    for dil in (1, 2):
        assert call(d_in=None, dil=dil) == EINVAL and call(packed=None, dil=dil) == EINVAL and call(out=None, dil=dil) == EINVAL
        assert call(in_max=None, dil=dil) == EINVAL and call(batch=0, dil=dil) == EINVAL and call(batch=-3, dil=dil) == EINVAL
        assert call(W=9, dil=dil) == EUNSUPPORTED and call(cin=24, dil=dil) == EUNSUPPORTED and call(cin=8, dil=dil) == EUNSUPPORTED
        assert call(D=0, dil=dil) == EUNSUPPORTED and call(cout=0, dil=dil) == EUNSUPPORTED
        # 2^31 units: 2^30 items x 2 units (7^3, 16 channels out)
        assert int(L.m3d_conv3d_zn_dilated_launch_units(1 << 30, 16, 16, 7, 7, 7, dil)) == 1 << 31
        assert call(batch=1 << 30, cin=16, dil=dil) == EUNSUPPORTED
    for dil in (0, 3, -1, 4):
        assert call(dil=dil) == EUNSUPPORTED
        assert call(d_in=None, dil=dil) == EINVAL                      # a NULL pointer is EINVAL whatever else is wrong


# ------------------------------------------------------------------ integers
@pytest.mark.parametrize("case", T.CASE_NAMES)
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_integer_operands_are_exact(direction, case):
    a, wl, shift = T.integer_inputs(case, direction)
    want = T.reference_op(direction, a, wl, None, shift)
    assert torch.equal(T.emulated(a, wl, shift=shift), want)
    _, al = T.cut(a, float(a.abs().max()))
    assert bool((al == 0).all())
    assert float(T.terms(T.conv_op, a, wl)[0].max()) < 2.0 ** 24


def test_exactly_zero_taps_of_the_thin_maps():
    """cout5 (D = 2), d1 (D = 1): every dz != 1 tap reads padding; w2: every dx != 1 tap; w3: dx = +-2 connects only x = 0 and x = 2"""
    for case, axis in (("cout5", 2), ("d1", 2), ("w2", 4)):
        a, wl, _ = T.integer_inputs(case, "forward")
        mid = torch.zeros_like(wl)
        idx = [slice(None)] * 5
        idx[axis] = 1
        mid[tuple(idx)] = wl[tuple(idx)]
        assert torch.equal(T.conv_op(a.double(), wl.double()), T.conv_op(a.double(), mid.double())), case
    a, wl, _ = T.integer_inputs("w3", "forward")
    side = torch.zeros_like(wl)
    side[..., 0], side[..., 2] = wl[..., 0], wl[..., 2]
    y = T.conv_op(a.double(), side.double())
    assert bool((y[..., 1] == 0).all()) and bool((y[..., 0] != 0).any()) and bool((y[..., 2] != 0).any())


# ------------------------------------------------------------------ random families: the correct kernel stays inside E
@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("case", T.CASE_NAMES)
def test_the_cut_meets_the_bound(case, family):
    for direction in T.DIRECTIONS:
        a, wl, scale, shift, relu, y, E, Cm = T.reference(case, direction, family)
        got = T.emulated(a, wl, scale, shift, relu)
        assert check(got, y, E), direction
        assert torch.equal(got[Cm == 0], y[Cm == 0])                       # a zero product is exact
        if direction == "dgrad":          # the launched conv on the flipped, transposed weight IS the transposed conv
            assert torch.allclose(T.finish(T.conv_op(a.double(), wl.double())), y, rtol=1e-9, atol=1e-12 * float(y.abs().max()) + 1e-300)


# ------------------------------------------------------------------ the cases can see a wrong kernel
def _seen(case, family="benign"):
    """the seeded defects and mutants that leave E on this case (forward form with its epilogue), and those that break integer exactness"""
    a, wl, scale, shift, relu, y, E, _ = T.reference(case, "forward", family)
    out = {m for m in T.CUT_MUTANTS if not check(T.emulated(a, wl, scale, shift, relu, mutant=m), y, E)}
    out |= {d for d in T.GEOMETRY_DEFECTS if not check(T.emulated(a, wl, scale, shift, relu, defect=d), y, E)}
    ai, wi, si = T.integer_inputs(case, "forward")
    want = T.reference_op("forward", ai, wi, None, si)
    ints = {d for d in T.GEOMETRY_DEFECTS if not torch.equal(T.emulated(ai, wi, shift=si, defect=d), want)}
    return out, ints


def test_every_seeded_defect_and_mutant_leaves_E_on_some_case():
    everything = set(T.CUT_MUTANTS) | set(T.GEOMETRY_DEFECTS)
    seen = {case: _seen(case) for case in T.CASE_NAMES}
    for name in everything:
        assert any(name in s for s, _ in seen.values()), name
    for d in T.GEOMETRY_DEFECTS:
        assert any(d in i for _, i in seen.values()), d
    # the RoI grid (7^3: a partial z tile behind a full one) sees every one of them, on random and on integer data
    assert seen["roi_grid"][0] == everything and seen["roi_grid"][1] == set(T.GEOMETRY_DEFECTS)
    # every cut mutant shows on every case; a one-voxel halo shows where a second z or y tile exists (its first row reads two below)
    for case, (s, _) in seen.items():
        assert set(T.CUT_MUTANTS) <= s, case
        _, _, _, D, H, _ = T.cases()[case]
        assert ("halo_1" in s) == (D > T.TILE_Z or H > T.TILE_Y), case
    # both sides of both tile edges: only `tiles` has a y tile behind another
    assert "halo_1" in seen["tiles"][0]


def test_scale_up_overflows_at_the_bound():
    a, wl, scale, shift, relu, y, E, _ = T.reference("roi_grid", "forward", "at_bound_below")
    assert not check(T.emulated(a, wl, scale, shift, relu, mutant="scale_up"), y, E)


# ------------------------------------------------------------------ the Python faces
def test_znconv3d_queries_take_the_dilation(L):
    from m3d import ops
    z = ops.ZnConv3d.__new__(ops.ZnConv3d)
    for cin, cout, (D, H, W), B in itertools.product((16, 32), (5, 64, 130), ((7, 7, 7), (14, 14, 8), (7, 7, 9), (1, 7, 3)), (1, 131)):
        z.cin, z.cout = cin, cout
        old = bool(L.m3d_conv3d_zn_supported(cin, cout, D, H, W))
        assert z.supports((D, H, W)) == old and z.supports((D, H, W), dilation=1) == old and z.supports((D, H, W), dilation=2) == old
        assert z.supports((D, H, W), dilation=3) is False
        assert not z.supports((D, H, W), pool=True, dilation=2)
        u = int(L.m3d_conv3d_zn_launch_units(B, cin, cout, D, H, W))
        assert z.units((B, cin, D, H, W)) == u == z.units((B, cin, D, H, W), dilation=1)
        assert z.units((B, cin, D, H, W), dilation=2) == int(L.m3d_conv3d_zn_dilated_launch_units(B, cin, cout, D, H, W, 2))


def test_the_switch_round_trips_and_install_leaves_it_off():
    import m3d.compat as c
    from m3d import conv_plan as P
    assert c.get_conv_dilated_f16() is False
    assert c.set_conv_dilated_f16(True) is False and c.get_conv_dilated_f16() is True and c._setting.dilated_f16 == P.ZN_DILATED_MIN_UNITS
    assert c.get_conv_dilated() == "torch"                                  # it does not turn the dilated route on by itself
    assert c.set_conv_dilated_f16(True, min_units=0) is True and c._setting.dilated_f16 == 0
    with pytest.raises(ValueError):
        c.set_conv_dilated_f16(True, min_units=-1)
    assert c.set_conv_dilated_f16(False) is True and c.get_conv_dilated_f16() is False
    c.install()
    try:
        assert c.get_conv_dilated_f16() is False
    finally:
        c.uninstall_conv3d()
        c.uninstall_linear()
