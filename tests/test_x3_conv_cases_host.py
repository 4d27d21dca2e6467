"""CPU: the case table of tests/x3_conv_cases.py meets its conditions for both forms of csrc/conv3d_x3.hip - asked of the library's own host
queries (m3d_conv3d_x3_workspace_bytes, m3d_conv3d_x3_launch_units), so that a moved split threshold or tile size fails here and not
silently on the GPU; every integer case is provably exact (the planes sum to the operands, the dropped products are zero, S < 2^24, every
kept product is live in every K range, chunk parity and row block, and the fp32 emulation equals fp64 bit for bit); every seeded defect
of the emulation is caught by the GPU test's comparison on every case it applies to; and the emulation stays inside the random-data bound."""
import numpy as np
import pytest
import torch

import x3_conv_cases as T


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d import ops
    assert (ops.W_PLAIN, ops.W_RELU) == (T.W_PLAIN, T.W_RELU)
    return ops.lib()


def of(form, cond=lambda c: True):
    return [c for c in T.CASES if c.form == form and cond(c)]


def split(c):
    """a case whose launch splits K"""
    return c.ksplit > 1


# ------------------------------------------------------------------ the table
def test_ksplit_is_the_librarys(L):
    assert len(set(T.CASES)) == len(T.CASES) == len({T.case_id(c) for c in T.CASES})
    for c in T.CASES:
        assert L.m3d_conv3d_x3_supported(c.cin, c.cout) == 1 and c.cin % 16 == 0
        by_ws, by_units = T.queried_ksplit(L, c)
        assert by_ws == by_units, (c, by_ws, by_units)
        assert by_ws == c.ksplit if c.ws else (c.ksplit == 1 and by_ws > 1), (c, by_ws)
        assert T.flop(c) <= T.CAP_FLOP, (c, T.flop(c))
        assert c.mode in (T.W_PLAIN, T.W_RELU)
        # the K ranges are whole chunk pairs, in order, and cover every chunk once
        r = T.k_ranges(c)
        assert r[0][0] == 0 and r[-1][1] == T.chunks_of(c) and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(c0 % 2 == 0 and c1 > c0 for c0, c1 in r)


@pytest.mark.parametrize("form", T.FORMS)
def test_conditions_of_every_form(L, form):
    lens = lambda c: [c1 - c0 for c0, c1 in T.k_ranges(c)]
    # K splits
    assert {c.ksplit for c in of(form)} == {1, 2, 4}
    assert of(form, lambda c: c.ksplit == 2 and c.cin in (80, 96) and T.pairs_of(c) % 2 == 1 and len(set(lens(c))) == 2)
    assert of(form, lambda c: c.ksplit == 4 and c.cin == 144 and lens(c) == [2, 2, 2, 3])
    assert of(form, lambda c: c.ksplit == 4 and c.cin == 128 and lens(c) == [2, 2, 2, 2])
    # unsplit runs
    un = lambda cond: of(form, lambda c: c.ksplit == 1 and cond(c))
    assert un(lambda c: c.cin == 16) and un(lambda c: c.cin == 32) and un(lambda c: c.cin == 48) and un(lambda c: c.cin >= 80)
    big = un(lambda c: c.ws and T.units(c) >= 192 and T.units(c) % 8 != 0 and T.pairs_of(c) >= 2 and T.elems(c) % 4 == 0)
    assert big and all(T.queried_ksplit(L, c, D=c.D // 2)[0] > 1 and T.units(c._replace(D=c.D // 2)) < 192 for c in big)     # only the unit count
    assert un(lambda c: T.units(c) < 8)
    odd = un(lambda c: c.ws and T.elems(c) % 4 != 0 and T.units(c) < 192)
    assert odd and all(T.queried_ksplit(L, c, W=c.W + c.W % 2)[0] > 1 for c in odd)                          # only the element count
    nows = un(lambda c: not c.ws)
    assert nows and all(T.queried_ksplit(L, c)[0] > 1 and c._replace(ws=True, ksplit=T.queried_ksplit(L, c)[0]) in T.CASES for c in nows)
    # tiles
    assert of(form, lambda c: min(T.tiles(c)) >= 2 and c.W % T.TX != 0 and c.H % T.TY != 0 and c.D % T.TZ != 0)
    assert of(form, lambda c: c.W < T.TX and c.H < T.TY and c.D < T.TZ and c.batch == 1)
    assert of(form, lambda c: c.W % 2 == 1)
    # channels
    assert of(form, lambda c: 0 < c.cout % 64 <= 32 and c.cout > 64) and of(form, lambda c: 32 < c.cout % 64 < 64)
    assert of(form, lambda c: c.cout < 32) and of(form, lambda c: c.cout > 64)
    # batch
    assert of(form, lambda c: c.batch == 2 and split(c)) and of(form, lambda c: c.batch == 2 and not split(c))
    # both modes, split and unsplit
    for mode in (T.W_PLAIN, T.W_RELU):
        assert of(form, lambda c: c.mode == mode and split(c)) and of(form, lambda c: c.mode == mode and not split(c))


def test_the_tile_sizes_are_the_librarys(L):
    """units(): one more voxel along an axis at a tile boundary adds a tile, one fewer does not"""
    lu = lambda B, cin, cout, D, H, W: int(L.m3d_conv3d_x3_launch_units(B, cin, cout, D, H, W))
    assert lu(1, 16, 64, 4, 4, 16) == 1 and lu(1, 16, 65, 4, 4, 16) == 2
    assert lu(1, 16, 64, 5, 4, 16) == 2 and lu(1, 16, 64, 4, 5, 16) == 2 and lu(1, 16, 64, 4, 4, 17) == 2 and lu(3, 16, 64, 4, 4, 16) == 3


# ------------------------------------------------------------------ exactness
def int_inputs(c, loose=False):
    x, w, off = T.integer_operands(c)
    return x, w, off, (T.in_max_of(c, x, off, loose) if c.form == "x3f" else None)


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_integer_case_is_exact(c):
    x, w, off = T.integer_operands(c)
    assert np.array_equal(x, np.rint(x)) and np.array_equal(w, np.rint(w))
    a, wr = T.operand_of(x, off), T.weights_of(c, w)
    if c.mode == T.W_RELU:
        assert off == T.INT_OFF == float(x.min()) and off != 0 and float(a.min()) == 0 and (w < 0).any() and float(wr.min()) == 0
    else:
        assert off is None and (x < 0).any() and (w < 0).any()
    y, S = T.integer_reference(c)
    assert float(S.max()) < 2.0 ** 24, float(S.max())
    assert float(S.min()) > 0 and (c.mode == T.W_RELU or bool((y < 0).any()))
    modes = (False, True) if c.form == "x3f" else (False,)
    for loose in modes:
        in_max = T.in_max_of(c, x, off, loose) if c.form == "x3f" else None
        A = T.a_bound(off, in_max) if c.form == "x3f" else None
        if c.form == "x3f":
            assert A == (T.F16_TWO + 3) * (256 if loose else 1) and T.w_bound(wr) == T.F16_TWO + 3
        assert T.cut_is_exact(c, a, wr, A)
        pa, pw = T.planes64(c, a, wr, A)
        # every kept (w piece, a piece) pair reaches some output in every K range, in both chunk parities, in both 32-row blocks
        ta, tw = [torch.from_numpy(np.abs(p)) for p in pa], [torch.from_numpy(np.abs(p)) for p in pw]
        for c0, c1 in T.k_ranges(c):
            for par in sorted({ch & 1 for ch in range(c0, c1)}):
                chans = [k for ch in range(c0, c1) if ch & 1 == par for k in range(16 * ch, 16 * ch + 16)]
                for r0 in range(0, c.cout, 32):
                    for iw, ia in T.PRODUCTS[c.form]:
                        live = T.DC.conv64(ta[ia][:, chans], tw[iw][r0:r0 + 32][:, chans], 3)
                        assert bool((live > 0).any()), (T.case_id(c), (c0, c1), par, r0, (iw, ia))
        for ksplit in sorted({c.ksplit, 1}):
            got = T.emulate(c, x, w, off, in_max, ksplit=ksplit)
            assert T.same_buffers(got, T.expected(c, y, ksplit)), (T.case_id(c), loose, ksplit)


def test_both_parities_exist_wherever_a_range_has_two_chunks():
    for c in T.CASES:
        for c0, c1 in T.k_ranges(c):
            assert c0 % 2 == 0 and ({ch & 1 for ch in range(c0, c1)} == {0, 1} or c1 - c0 == 1)


def test_cut_is_exact_tells_a_scale_that_is_not():
    """an in_max 2^30 above max x pushes the low plane of the two-plane probes below fp16's subnormals: the planes no longer sum to the
    operand and the emulation misses the reference"""
    c = next(c for c in T.CASES if c.form == "x3f" and c.cin == 16)
    x, w, off = T.integer_operands(c)
    in_max = float(np.float32(off) + np.float32((T.F16_TWO + 3) * 2.0 ** 30))
    assert not T.cut_is_exact(c, T.operand_of(x, off), T.weights_of(c, w), T.a_bound(off, in_max))
    assert not T.same_buffers(T.emulate(c, x, w, off, in_max), T.expected(c, T.integer_reference(c)[0]))


# ------------------------------------------------------------------ defects
@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_every_defect_is_caught_on_every_case_it_applies_to(c):
    """by the GPU test's own comparison: `out`, the guard rows behind it and behind the workspace against the fp64 reference, bit for bit"""
    x, w, off, in_max = int_inputs(c)
    want = T.expected(c, T.integer_reference(c)[0])
    missed = [d for d in T.DEFECTS if T.defect_applies(c, d) and T.same_buffers(T.emulate(c, x, w, off, in_max, defect=d), want)]
    assert not missed, (T.case_id(c), missed)


def test_defects_apply_where_they_should():
    for form in T.FORMS:
        ids = lambda d: {T.case_id(c) for c in of(form) if T.defect_applies(c, d)}
        every = {T.case_id(c) for c in of(form)}
        for d in ("stale_tap", "tap_z", "tap_y", "tap_x", "skip_first_chunk", "repeat_last_chunk", "first_flush_adds"):
            assert ids(d) == every, d
        for d in T.DEFECTS:
            if d.startswith("drop_"):
                assert ids(d) == (every if d in T._product_names(form) else set()), (form, d)
        assert ids("pad_minus_off") == {T.case_id(c) for c in of(form, lambda c: c.mode == T.W_RELU)}
        assert ids("reduce_skips_last") == {T.case_id(c) for c in of(form, split)}
        assert ids("upper_block_past_cout") == {T.case_id(c) for c in of(form, lambda c: c.cout % 64 != 0)}
        assert ids("colxy_swap") == {T.case_id(c) for c in of(form, lambda c: c.W >= 8)} and len(ids("colxy_swap")) >= len(every) - 1
    assert len(T._product_names("x3")) == 6 and len(T._product_names("x3f")) == 3 and set(T._product_names("x3f")) <= set(T.DEFECTS)


# ------------------------------------------------------------------ the bound
WORST = {}


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_emulation_stays_inside_the_bound_on_random_data(c):
    x, w, off = T.random_operands(c)
    a = T.operand_of(x, off)
    if c.mode == T.W_RELU:
        assert float(x.min()) == off and float(a.min()) == 0 and float(a.max()) > 0
        pos = a[a > 0]
        assert float(pos.max()) / float(pos.min()) >= 2.0 ** 16 or c.D * c.H * c.W < 100           # several decades
    else:
        assert (x < 0).any() and off is None
    for loose in ((False, True) if c.form == "x3f" else (False,)):
        in_max = T.in_max_of(c, x, off, loose) if c.form == "x3f" else None
        y, E, S = T.bound(c, x, w, off, in_max)
        got = torch.from_numpy(T.emulate(c, x, w, off, in_max).out[:T.elems(c)].astype(np.float64)).reshape(y.shape)
        assert bool(torch.isfinite(got).all())
        zero = S == 0
        assert bool(zero.any()) and bool((got[zero] == 0).all()) and bool((y[zero] == 0).all())
        assert torch.equal(got == 0, zero)          # zero exactly where every product is (f16x2: none of these outputs lies below the cut's floor)
        ratio = float(((got - y).abs() / E.clamp_min(1e-300)).max())
        key = (c.form, c.ksplit)
        WORST[key] = max(WORST.get(key, 0.0), ratio)
        assert ratio <= 1.0, (T.case_id(c), loose, ratio)
    print("x3 conv emulation: worst |got - y| / bound so far %s ksplit %d  %.4f" % (c.form, c.ksplit, WORST[(c.form, c.ksplit)]))
