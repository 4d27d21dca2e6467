"""GPU: every forward linear GEMM instance of csrc/fc_gemm.hip (seven kernel instantiations behind m3d_linear_forward, m3d_linear_bf16x3_forward,
m3d_linear_bf16x3_w32_forward and m3d_linear_f16x2_forward_bounds, and their common split-K reduce kernel) against fp64, element by element,
over the case table of tests/linear_cases.py.  That the table covers every instance at ragged tiles, uneven and one-chunk K slices, idle
workgroups, both slice counts of the fp32 kernel's tail path and every kept product of the split kernels, that the integer operands are
exact and that seeded defects are caught is proved on the CPU by tests/test_linear_cases_host.py.

 plan    inside the case's library context m3d_linear_plan names the tile and the slice counts of the table: a retuned planner that moves a
         case to another kernel fails here instead of silently testing that kernel twice;
 (a)     exact on integers: the output EQUALS the fp64 reference, plain and with integer bias and ReLU, and a second run is bit-identical;
         `out` is a view of a larger buffer full of a sentinel (one more row, one more element), which must survive; a mismatch names the
         tiles, the rows and columns inside a tile and the slice lengths;
 (b)     the f16x2 kernels under an exact, a loose (2^8) and a swept x bound, and the out_bound they leave: max |out| exactly;
 (c)     bounded on random data whose rows span 2^20 with zero rows among them: the per-element bound of linear_cases.bound; where nothing is
         summed the output is exactly the bias.  The worst ratio per instance is printed (pytest -s);
 routes  SplitLinear and SplitLinearF16 send up to 32 rows to the fp32 kernel, SplitLinear a few rows past a multiple of 256 as well (two
         launches into two slices of one `out`): exact on integers, with the seam rows checked.  (SplitLinearF16 has no row split.)

Largest measured |got - y| / bound per instance (MI355X), the record of (c) and no threshold:
    f32.full 0.0419  f32.tail1 0.0283  f32.tail2 0.0443  x3.128 0.0406  x3.256 0.0361  x3.w32 0.0343  f16.128 0.8351  f16.256 0.8298  f16.big 0.8623
The f16x2 figures are the last rounding alone: an output just above a power of two (y = 2.00001, a bias plus a sum 2^-11 of it) is half
an ulp = 2^-24 |y| off, which is the bound's last term; without bias the same kernels reach 0.23 at most, and the NumPy emulation of
tests/test_linear_cases_host.py gives the same figures on the same operands.  Every exact test passed.
"""
import contextlib
import functools

import numpy as np
import pytest
import torch

import linear_cases as T

pytestmark = pytest.mark.gpu

WORST = {}
RAN = set()


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    for inst in T.INSTANCES:
        print("linear forward: %-9s %s worst |got - y| / bound %s" % (inst, "ran" if inst in RAN else "DID NOT RUN",
                                                                         "%.4f" % WORST[inst] if inst in WORST else "-"))
    torch.cuda.empty_cache()


@contextlib.contextmanager
def library_for(ops, c):
    """the release library, or the tuning library with the case's options; either way the plan must be the one the table names"""
    from m3d import _lib
    with (_lib.tuning() if c.knobs else contextlib.nullcontext()):
        for name, v in c.knobs:
            _lib.set_option(name, v)
        got = ops.linear_plan(T.kind_of(c), c.M, c.N, c.K)
        assert got == T.expected_plan(c), "%s: planned %s, the table names %s" % (T.case_id(c), got, T.expected_plan(c))
        RAN.add(c.inst)
        yield


def layer_of(ops, c, w, bias):
    """callable(x, relu, out, **bounds) of the case's entry point on device operands"""
    fam = T.family(c)
    if fam == "f32":
        return lambda x, relu, out: ops.linear(x, w, bias, relu=relu, out=out)
    if fam == "x3":
        lin = ops.SplitLinear(w, bias)
        variant = "w32" if c.inst == "x3.w32" else "packed"
        return lambda x, relu, out: lin(x, relu=relu, out=out, variant=variant)
    assert c.M > 32                                                   # SplitLinearF16 sends fewer rows to the fp32 kernel
    lin = ops.SplitLinearF16(w, bias)
    return lambda x, relu, out, **kw: lin(x, relu=relu, out=out, **kw)


def run(call, M, N, *a, **kw):
    """the call on `out` = the first M * N elements of a sentinel-filled buffer of (M + 1) * N + 1; returns the whole buffer (CPU, numpy)"""
    buf = torch.full(((M + 1) * N + 1,), T.SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[:M * N].view(M, N)
    res = call(*a, out=out, **kw)
    assert res.data_ptr() == out.data_ptr()
    return buf.cpu().numpy()


def same(c, got, ref, what):
    """the buffer equals the fp64 reference cast to fp32 inside `out` and the sentinel outside it; on a mismatch: how many, the first and
    the last, the tiles, the rows and the columns within a tile (they name the wave and the lane group), and the slice lengths of the case
    (a slice cannot be told from the output)"""
    want = T.expected_buffer(ref)
    assert got.shape == want.shape
    if np.array_equal(got, want):
        return
    M, N = ref.shape
    tr, tc = T.TILE[c.inst]
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))
    inside = bad[bad < M * N]
    rows, cols = inside // N, inside % N

    def el(i):
        return "(%d, %d) got %r want %r" % (i // N, i % N, float(got[i]), float(want[i]))
    raise AssertionError(
        "%s %s: %d of %d elements differ, %d of them sentinels behind out; first %s; last %s; tiles (row, column) %s; rows in tile %s; "
        "columns in tile %s; slice lengths %s (row groups %s)"
        % (T.case_id(c), what, bad.size, M * N, bad.size - inside.size, el(bad[0]), el(bad[-1]),
           sorted(set(zip((rows // tr).tolist(), (cols // tc).tolist())))[:16], sorted(set((rows % tr).tolist()))[:40],
           sorted(set((cols % tc).tolist()))[:40], T.slice_lengths(c), [(r0, r1) for r0, r1, _ in T.row_groups(c)]))


@functools.lru_cache(maxsize=None)
def integer_reference(fam, M, N, K):
    """operands and fp64 references of a family and shape, shared by its cases and left unchanged"""
    c = next(c for c in T.CASES if (T.family(c), c.M, c.N, c.K) == (fam, M, N, K))
    x, w, b = T.integer_operands(c)
    out = (x, w, b, T.reference(x, w), T.reference(x, w, b, relu=True))
    for a in out:
        a.setflags(write=False)
    return out


def dev(a):
    return torch.from_numpy(np.array(a, copy=True)).cuda()          # a copy: the shared references are read-only


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_exact_on_integers(ops, c):
    x, w, b, ref, refb = integer_reference(T.family(c), c.M, c.N, c.K)
    xd, wd, bd = dev(x), dev(w), dev(b)
    with library_for(ops, c):
        plain, biased = layer_of(ops, c, wd, None), layer_of(ops, c, wd, bd)
        got = run(plain, c.M, c.N, xd, False)
        same(c, got, ref, "plain")
        gotb = run(biased, c.M, c.N, xd, True)
        same(c, gotb, refb, "bias, relu")
        assert np.array_equal(run(plain, c.M, c.N, xd, False), got) and np.array_equal(run(biased, c.M, c.N, xd, True), gotb)


@pytest.mark.parametrize("c", [c for c in T.CASES if T.family(c) == "f16"], ids=T.case_id)
def test_f16x2_bounds_on_integers(ops, c):
    """x_bound exact, loose by 2^8 and swept by the library, each where the cut stays exact under that scale (linear_cases.cut_is_exact,
    which the host test holds against the emulation); the zeroed out_bound receives max |out| exactly - from the GEMM's epilogue
    (slices == 1) or from the reduce kernel"""
    x, w, b, ref, refb = integer_reference("f16", c.M, c.N, c.K)
    xd, wd, bd = dev(x), dev(w), dev(b)
    amax = float(np.abs(x).max())
    ran = 0
    with library_for(ops, c):
        plain, biased = layer_of(ops, c, wd, None), layer_of(ops, c, wd, bd)
        for what, xb in (("exact", amax), ("loose", amax * 2.0 ** 8), ("swept", None)):
            if not T.cut_is_exact(c, x, w, xb):
                continue
            ran += 1
            for call, relu, want in ((plain, False, ref), (biased, True, refb)):
                ob = torch.zeros((ops.ZwConv3d.SLOTS,), dtype=torch.float32, device="cuda")
                kw = dict(out_bound=ob) if xb is None else dict(out_bound=ob, x_bound=torch.tensor([xb], dtype=torch.float32, device="cuda"))
                same(c, run(call, c.M, c.N, xd, relu, **kw), want, "x_bound %s, relu %d" % (what, relu))
                assert float(ob.max()) == float(np.abs(want).max()) and float(ob.min()) >= 0, (T.case_id(c), what, ob.tolist(), np.abs(want).max())
    assert ran == 3, ran                                             # by construction all three scales are exact (the module docstring)


def within(c, what, got, y, E, S):
    got = got[:c.M * c.N].reshape(c.M, c.N).astype(np.float64)
    assert np.isfinite(got).all()
    zero = S == 0
    assert np.array_equal(got[zero], y[zero]), (T.case_id(c), what, "an output with nothing to sum is not exactly the bias")
    r = np.abs(got - y) / np.maximum(E, 1e-300)
    ratio = float(r.max())
    WORST[c.inst] = max(WORST.get(c.inst, 0.0), ratio)
    i = np.unravel_index(int(r.argmax()), r.shape)
    print("linear forward ratio: %s %s %.4f at %s" % (T.case_id(c), what, ratio, i))
    tr, tc = T.TILE[c.inst]
    assert ratio <= 1.0, (T.case_id(c), what, ratio, "element", i, "tile", (i[0] // tr, i[1] // tc), "got", got[i], "y", y[i], "bound", E[i],
                          "elements over the bound", int((r > 1).sum()))


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_bounded_on_random_data(ops, c):
    x, w, b = T.random_operands(c)
    xd, wd, bd = dev(x), dev(w), dev(b)
    with library_for(ops, c):
        plain, biased = layer_of(ops, c, wd, None), layer_of(ops, c, wd, bd)
        for call, bias, relu in ((plain, None, False), (biased, b, True)):
            y, E, S = T.bound(c, x, w, bias, relu)
            got = run(call, c.M, c.N, xd, relu)
            assert np.array_equal(got[c.M * c.N:], T.expected_buffer(y)[c.M * c.N:])
            within(c, "relu %d" % relu, got, y, E, S)
        if T.family(c) == "f16":                                     # a bound 2^8 above max |x|: its own (wider) contract bound
            A = float(np.abs(x).max()) * 2.0 ** 8
            y, E, S = T.bound(c, x, w, b, True, x_bound=A)
            within(c, "relu 1, loose x bound", run(biased, c.M, c.N, xd, True, x_bound=torch.tensor([A], dtype=torch.float32, device="cuda")), y, E, S)


# ------------------------------------------------------------------ the routes of the Python classes
ROUTE_N, ROUTE_K = 130, 160


@functools.lru_cache(maxsize=None)
def route_operands(fam, M):
    c = T.Case(fam + ".256", M, ROUTE_N, ROUTE_K, 1, 1, ())
    x, w, b = T.integer_operands(c)
    assert float(T.magnitude(x, w, b).max()) < 2.0 ** 24 and T.cut_is_exact(c, x, w)
    return c, x, w, b, T.reference(x, w, b, relu=True)


@pytest.mark.parametrize("M", (1, 31, 32, 33))
@pytest.mark.parametrize("fam", ("x3", "f16"))
def test_few_rows_route_is_exact(ops, monkeypatch, fam, M):
    """M <= 32 goes to the fp32 kernel (its tail path: no full tile), 33 rows are the split kernel's first"""
    c, x, w, b, ref = route_operands(fam, M)
    calls = []
    real = ops.linear
    monkeypatch.setattr(ops, "linear", lambda x_, *a, **kw: calls.append(int(x_.shape[0])) or real(x_, *a, **kw))
    lin = (ops.SplitLinear if fam == "x3" else ops.SplitLinearF16)(dev(w), dev(b))
    got = run(lambda x_, out: lin(x_, relu=True, out=out), M, ROUTE_N, dev(x))
    assert calls == ([M] if M <= 32 else [])
    same(c, got, ref, "rows %d" % M)


@pytest.mark.parametrize("M,tail", ((513, 1), (576, 64), (577, 0), (512, 0)))
def test_row_split_route_is_exact(ops, monkeypatch, M, tail):
    """SplitLinear, M > 512 with 0 < M % 256 <= 64: the head through the packed kernel, the last M % 256 rows through the fp32 kernel, two
    launches into two row ranges of one `out` - the rows on both sides of the seam must be right and nothing behind `out` touched"""
    c, x, w, b, ref = route_operands("x3", M)
    calls = []
    real = ops.linear
    monkeypatch.setattr(ops, "linear", lambda x_, *a, **kw: calls.append(int(x_.shape[0])) or real(x_, *a, **kw))
    lin = ops.SplitLinear(dev(w), dev(b))
    got = run(lambda x_, out: lin(x_, relu=True, out=out), M, ROUTE_N, dev(x))
    assert calls == ([tail] if tail else [])
    same(c, got, ref, "rows %d = %d + %d" % (M, M - tail, tail))
