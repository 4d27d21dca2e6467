"""GPU: every stage of the peak-response back-propagation against its own fp64 reference, element by element, over the case tables of
tests/prm_stage_cases.py (that the references are the reference's rule, which kernel a case runs and that the table covers all of them is
proved on the CPU by tests/test_prm_stage_cases_host.py).  Per case:

 (a) exact: integer-valued data, exactly representable divisors, every partial sum below 2^24 - the result must EQUAL the fp64 reference
     bit for bit at every element, every column of a strip included (outputs are pre-filled with NaN: an unwritten separator shows);
 (b) bounded: random data over several decades with the cut edges of norm and xnext sprinkled in - the per-element bounds derived in
     prm_stage_cases' docstring; no band, no excluded voxels.  The worst |got - y| / bound is printed per case and per stage (pytest -s)."""

import numpy as np
import pytest
import torch

import prm_stage_cases as T

pytestmark = pytest.mark.gpu

F32, F64 = T.F32, T.F64
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    for stage, r in sorted(WORST.items()):
        print("prm stages: worst |got - y| / bound  %-22s %.4f" % (stage, r))
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def stop_after_a_gpu_error():
    """a device error (a fault in a kernel under test) ends the run: nothing more is launched on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("GPU error, no further launches: %s" % e, returncode=3)


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def scalar(v):
    return None if v is None else torch.tensor([float(v)], dtype=torch.float32, device="cuda")


def host(t):
    return t.cpu().numpy()


def note(stage, what, r):
    WORST[stage] = max(WORST.get(stage, 0.0), r)
    print("prm stage ratio: %-22s %-60s %.4f" % (stage, what, r))
    assert r <= 1.0, (stage, what, r)


# ------------------------------------------------------------------ prepare: the five kernels
def run_prepare(ops, c, inp, gin, P=3):
    """m3d_prm_prepare_ex3 on the case's layouts; out, origins and the peak maxima pre-filled, so that what the launch leaves unwritten shows"""
    from m3d._lib import lib, check
    assert ops.prm_prepare_plan(c.C, P, c.U, c.pool, c.border, c.out_l, c.out_slab, c.shape[0]) == c.kernel
    Wn = (2 if c.pool else 1) * c.U + 2 * c.border
    shape = (c.C, c.shape[0] if c.out_slab else Wn, Wn, T.strip_geometry(Wn, c.out_l, P)[2]) if c.out_l else (P, c.C, Wn, Wn, Wn)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    assert out.data_ptr() % 16 == 0
    oo = torch.full((P, 3), -12345, dtype=torch.int32, device="cuda")
    pm = torch.full((P, 32), float("nan"), dtype=torch.float32, device="cuda")
    t = dict(gup=dev(gin), origin_up=dev(inp["origin_up"]), argmax=dev(inp["argmax"]), xnext=dev(inp["xnext"]), scale=dev(inp["scale"]),
             norm=dev(inp["norm"]), up_off=scalar(inp["up_off"]))
    up = inp["xnext"].shape[1:]
    p = ops._ptr
    check(lib().m3d_prm_prepare_ex3(p(t["gup"]), p(t["origin_up"]), P, c.C, c.U, int(c.pool), c.border, p(t["argmax"]), p(t["xnext"]),
                                    up[0], up[1], up[2], p(t["scale"]), p(t["norm"]), c.shape[0], c.shape[1], c.shape[2], c.in_l,
                                    int(c.in_slab), c.out_l, int(c.out_slab), p(t["up_off"]), p(out), p(oo), p(pm), ops._stream()),
          "prm_prepare")
    return host(out), host(oo), host(pm)


def check_peak_max(c, got, origin_out, pm, P=3):
    """peak_max[32 p] is max |window p| of what was written, bit for bit; the rest of each peak's cache line is the zero fill"""
    Wn = (2 if c.pool else 1) * c.U + 2 * c.border
    win = T.unpack_strip(got, c.out_l, P, Wn, origin_out[:, 0] if c.out_slab else None)
    want = np.abs(win).reshape(P, -1).max(1).astype(F32)
    T.same_bits(pm[:, 0], want, "peak_max")
    assert not pm[:, 1:].any()


@pytest.mark.parametrize("c", T.PREP_CASES, ids=T.prep_id)
def test_prepare_exact(ops, c):
    inp = T.prep_inputs(c, True)
    y, o = T.prep_reference(c, inp)
    assert np.abs(y).max() < T.LIMIT
    gin, want = T.prep_layouts(c, inp, y, o)
    got, oo, pm = run_prepare(ops, c, inp, gin)
    assert np.array_equal(oo, o)
    T.same_bits(got, want, T.prep_id(c))
    check_peak_max(c, got, o, pm)


@pytest.mark.parametrize("c", T.PREP_CASES, ids=T.prep_id)
def test_prepare_bounded(ops, c):
    inp = T.prep_inputs(c, False)
    y, o = T.prep_reference(c, inp)
    gin, want = T.prep_layouts(c, inp, y, o)
    bound = T.prep_layouts(c, inp, T.bound_pointwise(y, T.k_prepare(c.up_off, c.scale)), o)[1]
    got, oo, pm = run_prepare(ops, c, inp, gin)
    assert np.array_equal(oo, o)
    note("prepare " + c.kernel, T.prep_id(c), T.ratio(got, want, bound, T.prep_id(c)))
    check_peak_max(c, got, o, pm)


def test_prepare_through_the_wrapper_and_unaligned(ops):
    """ops.prm_prepare (what the engine calls) gives the raw call's bits; an output that is not 16-byte aligned runs the element kernel on
    the quad-aligned strip and writes the same strip"""
    from m3d._lib import lib, check
    c = next(c for c in T.PREP_CASES if c.kernel == "quad<8>" and c.U == 14 and c.border == 2 and not c.in_l)
    inp = T.prep_inputs(c, True)
    y, o = T.prep_reference(c, inp)
    gin, want = T.prep_layouts(c, inp, y, o)
    got, oo = ops.prm_prepare(dev(gin), dev(inp["origin_up"]), c.pool, c.border, None, dev(inp["xnext"]), dev(inp["scale"]), dev(inp["norm"]),
                              in_strip=c.in_l, out_strip=c.out_l, up_off=scalar(inp["up_off"]), dims=(3, c.C, c.U), in_slab=c.in_slab,
                              out_slab=c.out_slab, peak_max=True)
    T.same_bits(host(got), want, "wrapper")
    check_peak_max(c, host(got), o, host(got._m3d_peak_max))
    buf = torch.full((want.size + 4,), float("nan"), dtype=torch.float32, device="cuda")
    out = buf[1:1 + want.size]
    assert out.data_ptr() % 16 == 4
    oo = torch.empty((3, 3), dtype=torch.int32, device="cuda")
    t = [dev(gin), dev(inp["origin_up"]), dev(inp["xnext"]), dev(inp["scale"]), dev(inp["norm"]), scalar(inp["up_off"])]
    p = ops._ptr
    check(lib().m3d_prm_prepare_ex3(p(t[0]), p(t[1]), 3, c.C, c.U, 0, c.border, None, p(t[2]), c.shape[0], c.shape[1], c.shape[2], p(t[3]),
                                    p(t[4]), c.shape[0], c.shape[1], c.shape[2], c.in_l, int(c.in_slab), c.out_l, int(c.out_slab), p(t[5]),
                                    p(out), p(oo), None, ops._stream()), "prm_prepare")
    b = host(buf)
    T.same_bits(b[1:1 + want.size].reshape(want.shape), want, "unaligned")
    assert np.isnan(b[0]) and np.isnan(b[1 + want.size:]).all()         # nothing written around the strip


# ------------------------------------------------------------------ seed, den_pool, scatter
@pytest.mark.parametrize("c", T.SEED_CASES, ids=str)
def test_seed(ops, c):
    for exact in (True, False):
        e = T.seed_inputs(c, exact)
        y, o = T.ref_seed(e["peaks"], e["prob"], e["ncls"], e["wcls"], e["h"], e["off"])
        got, oo = ops.prm_seed(dev(e["peaks"]), dev(e["prob"]), dev(e["ncls"]), dev(e["wcls"]), dev(e["h"]), scalar(e["off"]), return_origin=True)
        assert tuple(got.shape) == (c.P, c.C, 1, 1, 1) and np.array_equal(host(oo), o)
        got = host(got).reshape(c.P, c.C)
        if exact:
            T.same_bits(got, y, "seed")
        else:
            note("seed", str(c), T.ratio(got, y, T.bound_pointwise(y, 9), "seed"))


@pytest.mark.parametrize("case", T.DEN_CASES, ids=str)
def test_den_pool(ops, case):
    for exact in (True, False):
        e = T.den_inputs(case, exact)
        y = T.ref_den_pool(e["argmax"], e["xnext"], e["norm"])
        got = host(ops.prm_den_pool(dev(e["argmax"]), dev(e["xnext"]), dev(e["norm"])))
        if exact:
            T.same_bits(got, y, "den_pool")
        else:
            note("den_pool", str(case), T.ratio(got, y, T.bound_pointwise(y, 1), "den_pool"))


@pytest.mark.parametrize("c", T.SCATTER_CASES, ids=str)
def test_scatter(ops, c):
    from m3d._lib import lib, check
    for exact in (True, False):
        e = T.scatter_inputs(c, exact)
        y = T.ref_scatter(e["win"], e["sums"], e["origin"], c.shape)
        assert np.isnan(y[3]).all() and not np.isnan(y[:3]).any()        # the zero sum: 0 / 0 at every voxel of that map only
        P = e["win"].shape[0]
        dense = torch.full((P,) + c.shape, -7777.0, dtype=torch.float32, device="cuda")
        t = [dev(e["win"]), dev(e["sums"]), dev(e["origin"])]
        check(lib().m3d_prm_scatter(ops._ptr(t[0]), ops._ptr(t[1]), ops._ptr(t[2]), P, c.win, c.shape[0], c.shape[1], c.shape[2],
                                    ops._ptr(dense), ops._stream()), "prm_scatter")
        got = host(dense)
        assert not (got == -7777.0).any()
        if exact:
            T.same_bits(got, y, "scatter")
            T.same_bits(host(ops.prm_scatter(t[0], t[1], t[2], c.shape)), y, "scatter wrapper")
        else:
            note("scatter", str(c), T.ratio(got, y, T.bound_pointwise(y, T.DIV), "scatter"))


# ------------------------------------------------------------------ windowed direct conv + PreHook, small-window GEMM (fp32)
def run_dgrad(ops, c, e):
    t = dict(gn=dev(e["gn"]), full=dev(e["full"]), off=scalar(e["off"]), origin=dev(e["origin"]))
    if c.variant is None:
        small = ops.SmallWindowDgrad(dev(e["w"]), f16=False)
        assert not small.f16
        return host(small(t["gn"], t["full"], t["off"], t["origin"]))
    assert ops.conv3d_direct_plan(c.P, c.cg, c.cx, c.win, c.win, c.win, 3)["variant"] == c.variant
    pack = ops.PackedConv3d(dev(e["w"]), ops.W_DGRAD_RELU)
    assert (pack.cin, pack.cout) == (c.cg, c.cx)
    return host(ops.conv3d_windowed(pack, t["gn"], t["full"], t["off"], t["origin"]))


@pytest.mark.parametrize("c", T.WINDOWED_CASES + T.SMALL_CASES, ids=T.dgrad_id)
def test_dgrad_prehook(ops, c):
    stage = "small GEMM fp32" if c.variant is None else "windowed conv"
    e = T.dgrad_inputs(c, True)
    y, ca = T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], want_cabs=True)
    assert ca.max() < T.LIMIT
    T.same_bits(run_dgrad(ops, c, e), y, T.dgrad_id(c), sums=True)          # every peak, every channel, every voxel
    e = T.dgrad_inputs(c, False)
    y, ca = T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], want_cabs=True)
    note(stage, T.dgrad_id(c), T.ratio(run_dgrad(ops, c, e), y, T.bound_sum(y, ca, 27 * c.cg), T.dgrad_id(c), signs=False))


# ------------------------------------------------------------------ stem: VALU form and the fused MFMA form, with the per-peak sums
@pytest.mark.parametrize("c", T.STEM_CASES, ids=str)
def test_stem_valu(ops, c):
    assert ops.prm_stem_dgrad_plan(c.win) == c.layout
    for exact in (True, False):
        e = T.stem_inputs(c, exact)
        y, s, ca = T.ref_stem(e["gn"], e["w"], e["data"], e["off"], e["origin"], want_cabs=True)
        wf = ops.prm_stem_prepare_weights(dev(e["w"]))
        got, gs = ops.prm_stem_dgrad(dev(e["gn"]), wf, dev(e["data"]), scalar(e["off"]), dev(e["origin"]))
        got, gs = host(got), host(gs)
        if exact:
            assert ca.max() < T.LIMIT and s.max() < T.LIMIT
            want_wf = np.maximum(e["w"].reshape(c.C, 125)[:, ::-1], 0)
            T.same_bits(host(wf), want_wf, "flipped relu(W)")
            T.same_bits(got, y, str(c), sums=True)
            T.same_bits(gs, s, "per-peak sums")
        else:
            b = T.bound_sum(y, ca, 125 * c.C, clamped=True)
            note("stem VALU " + c.layout, str(c), T.ratio(got, y, b, str(c), signs=False))
            note("stem VALU sums", str(c), T.ratio_sums(gs, got, y, b, c.win ** 3, str(c)))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("c", T.FUSED_CASES, ids=T.fused_id)
def test_stem_fused(ops, c, exact):
    assert ops.prm_stem_dgrad_fused_supported(32, c.U)
    inp, y, s, o, ca = T.fused_reference(c, exact)
    gin = T.pack_strip(inp["gup"], c.in_l, inp["origin_up"][:, 0] if c.slab else None, c.pooled[0] if c.slab else None)
    wa = ops.prm_stem_mfma_weights(dev(inp["w"]))
    got, gs, oo = ops.prm_stem_dgrad_fused(dev(gin), dev(inp["origin_up"]), dev(inp["den"]), dev(inp["argmax"]), dev(inp["scale"]), wa,
                                           dev(inp["data"]), scalar(inp["off"]), strip=c.in_l, xnext=dev(inp["xnext"]),
                                           up_off=scalar(inp["up_off"]), dims=(c.P, 32, c.U), slab=c.slab)
    got, gs = host(got), host(gs)
    assert np.array_equal(host(oo), o)
    if exact:
        assert ca.max() < T.LIMIT and s.max() < T.LIMIT
        T.same_bits(got, y, T.fused_id(c), sums=True)
        T.same_bits(gs, s, "per-peak sums")
    else:
        b = T.bound_sum(y, ca, 125 * 32, T.k_fused(c.up_off, c.scale), clamped=True)
        note("stem fused U=%d" % c.U, T.fused_id(c), T.ratio(got, y, b, T.fused_id(c), signs=False))
        note("stem fused sums", T.fused_id(c), T.ratio_sums(gs, got, y, b, (2 * c.U + 4) ** 3, T.fused_id(c)))
