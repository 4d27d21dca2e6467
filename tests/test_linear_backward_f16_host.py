"""CPU: the f16x2 linear backward's accuracy contract (tests/linear_backward_f16_cases.py) holds for the exact-sum emulation of the cut
and catches the four mutants; the library's host functions (_supported, _plan, workspace sizes, refusals) equal their documented rules;
the planner routes only what it should.  No GPU is touched: the entry points refuse before any pointer is followed."""
import ctypes as C
import itertools

import pytest

import linear_backward_f16_cases as LC

EINVAL, EUNSUPPORTED = -1, -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


# ------------------------------------------------------------------ the contract against the emulation
@pytest.mark.parametrize("kind", LC.KINDS)
@pytest.mark.parametrize("M,N,K", LC.CASES)
def test_emulation_meets_the_contract(M, N, K, kind):
    """the exact sum of the three products is inside the bound for ANY plan: n_acc = 0"""
    c = LC.case(M, N, K, kind)
    for name in ("dgrad", "wgrad"):
        y, E, Cm = LC.contract(c, name, 0)
        got = LC.emulate(c, name)
        r = LC.worst_ratio(got, y, E)
        print("(%d,%d,%d) %s %s: emulation, largest error / E = %.3f" % (M, N, K, kind, name, r))
        assert LC.violations(got, y, E) == 0, (name, r)
        assert bool((got[Cm == 0] == 0).all()), name


# (mutant, case, family) at which the mutant must leave the bound, at the LARGEST n_acc any plan of the cases has (a looser bound than
# the kernel is held to)
MUTANT_SITES = [("hi_only", (36, 64, 128), "benign"), ("hi_only", (77, 96, 160), "heavy"), ("drop_hilo", (36, 64, 128), "benign"),
                ("drop_hilo", (77, 96, 160), "quiet"), ("lo_unscaled", (36, 64, 128), "heavy"), ("lo_unscaled", (77, 96, 160), "benign"),
                ("scale_up", (36, 64, 128), "at_bound_below"), ("scale_up", (77, 96, 160), "at_bound_below")]


@pytest.mark.parametrize("mutant,shape,kind", MUTANT_SITES)
def test_mutants_violate_the_contract(mutant, shape, kind):
    c = LC.case(*shape, kind)
    nacc = 2 * LC.MAX_CHAIN + 2 + 64 + 2
    for name in ("dgrad", "wgrad"):
        y, E, _ = LC.contract(c, name, nacc)
        assert LC.violations(LC.emulate(c, name, mutant), y, E) > 0, (mutant, name)


def test_every_mutant_is_named():
    assert {m for m, _, _ in MUTANT_SITES} == set(LC.MUTANTS)


def test_scale_up_is_harmless_at_a_power_of_two():
    """at_bound_pow2: the bound 2^j scales to exactly 2^14, one more doubling still fits fp16 - the mutant shows only just below"""
    c = LC.case(36, 64, 128, "at_bound_pow2")
    for name in ("dgrad", "wgrad"):
        y, E, _ = LC.contract(c, name, 0)
        assert LC.violations(LC.emulate(c, name, "scale_up"), y, E) == 0


# ------------------------------------------------------------------ the host functions against a restatement of their rules
def supported_rule(M, N, K):
    return (M >= 1 and N >= 64 and K >= 4 and N % 4 == 0 and K % 4 == 0 and M * N < 2 ** 31 and N * K < 2 ** 31 and M * K < 2 ** 31)


def plan_rule(rows, red, K):
    """fc_backward_f16.hip make_plan: 128 x 128 tiles, 32-deep chunks, 512 workgroup slots, at most 64 slices of about four chunks or
    more, no split below 2^24 multiply-adds; 6 MFMAs per chunk, a fold every 64 chunks"""
    rt, kt, chunks = -(-rows // 128), -(-K // 128), -(-red // 32)
    tiles = rt * kt
    s = 1 if tiles >= 512 else 512 // tiles
    s = min(s, 64, chunks // 4 + 1)
    if rows * red * K < 2 ** 24:
        s = 1
    cps = -(-chunks // s)
    return dict(slices=s, chain=6 * min(cps, 64), folds=-(-cps // 64) if cps > 64 else 0)


SWEEP = list(itertools.product((1, 2, 31, 32, 33, 127, 128, 129, 300, 2049, 4100), (2, 12, 60, 64, 66, 68, 128, 1024, 2052, 4160),
                               (2, 4, 30, 64, 128, 132, 1000, 2744, 87808)))


def plans(L, M, N, K):
    out = []
    for fn in (L.m3d_linear_dgrad_f16x2_plan, L.m3d_linear_wgrad_f16x2_plan):
        v = [C.c_int(-7) for _ in range(3)]
        rc = fn(M, N, K, *[C.byref(a) for a in v])
        out.append((rc, dict(zip(("slices", "chain", "folds"), (a.value for a in v)))))
    return out


def test_supported_and_plan_equal_their_rules(L):
    for M, N, K in LC.CASES + SWEEP + [(128, 1024, 87808), (256, 1024, 43904), (512, 1024, 87808), (1, 64, 2 ** 25), (2 ** 20, 4096, 4)]:
        want = supported_rule(M, N, K)
        assert bool(L.m3d_linear_backward_f16x2_supported(M, N, K)) == want, (M, N, K)
        (rd, pd), (rw, pw) = plans(L, M, N, K)
        if not want:
            assert rd == rw == EUNSUPPORTED, (M, N, K)
            assert L.m3d_linear_dgrad_f16x2_workspace_bytes(M, N, K) == 0 and L.m3d_linear_wgrad_f16x2_workspace_bytes(M, N, K) == 0
            continue
        assert rd == rw == 0
        assert pd == plan_rule(M, N, K), (M, N, K, pd)
        assert pw == plan_rule(N, M, K), (M, N, K, pw)
        for p in (pd, pw):
            assert 1 <= p["slices"] <= 64 and 6 <= p["chain"] <= LC.MAX_CHAIN and p["folds"] >= 0
        assert L.m3d_linear_dgrad_f16x2_workspace_bytes(M, N, K) == 256 + (pd["slices"] * M * K * 4 if pd["slices"] > 1 else 0)
        assert L.m3d_linear_wgrad_f16x2_workspace_bytes(M, N, K) == 256 + (pw["slices"] * (N * K + N) * 4 if pw["slices"] > 1 else 0)
    assert L.m3d_linear_dgrad_f16x2_plan(0, 64, 64, None, None, None) == EINVAL
    assert L.m3d_linear_wgrad_f16x2_plan(4, 0, 64, None, None, None) == EINVAL
    assert L.m3d_linear_dgrad_f16x2_plan(4, 64, 64, None, None, None) == 0          # any output pointer may be NULL


def test_the_cases_reach_what_they_are_for(L):
    """the split, the fold and the ragged tiles the case table names are what the plans say"""
    def plan(M, N, K):
        return [p for _, p in plans(L, M, N, K)]
    assert plan(33, 1024, 1024)[0]["slices"] > 1
    assert plan(260, 128, 4096)[1]["slices"] > 1
    d, w = plan(40, 2112, 64)
    assert d["chain"] == LC.MAX_CHAIN and d["folds"] >= 1 and w["folds"] == 0
    d, w = plan(2100, 64, 64)
    assert w["chain"] == LC.MAX_CHAIN and w["folds"] >= 1 and d["folds"] == 0
    for M, N, K in ((128, 1024, 87808), (256, 1024, 43904), (512, 1024, 87808), (256, 1024, 1024)):      # the box head never folds
        assert all(p["folds"] == 0 for p in plan(M, N, K))


def test_refusals_follow_no_pointer(L):
    """every pointer NULL (and, where one is needed to get past the NULL check, a pointer nothing may follow): the refusal is the return code"""
    z, bad = C.c_void_p(0), C.c_void_p(16)
    sz = C.c_size_t(1 << 30)
    dg = lambda M, N, K, p=z: L.m3d_linear_dgrad_f16x2(p, p, p, M, N, K, z, 0, z, 0, p, sz, z)
    wg = lambda M, N, K, p=z: L.m3d_linear_wgrad_f16x2(p, p, p, z, M, N, K, z, 0, z, 0, p, sz, z)
    for f in (dg, wg):
        assert f(-1, 64, 64) == EINVAL and f(4, 0, 64) == EINVAL and f(4, 64, 0) == EINVAL
        for M, N, K in ((4, 2, 1024), (4, 12, 1024), (4, 66, 64), (4, 64, 66), (4, 60, 64), (2 ** 20, 4096, 64)):
            assert f(M, N, K) == EUNSUPPORTED, (M, N, K)
            assert f(M, N, K, bad) == EUNSUPPORTED, (M, N, K)
        assert f(4, 64, 64) == EINVAL                                              # supported shape, NULL operands
    assert dg(0, 64, 64) == 0                                                      # as m3d_linear_dgrad: nothing to do
    assert wg(0, 64, 64) == EINVAL                                                 # as m3d_linear_wgrad: d_gw is needed to zero it
    assert wg(0, 2, 64) == EUNSUPPORTED
    # slots outside 1..1024, a misaligned pointer, a workspace that is too small: refused with pointers nothing may follow
    assert L.m3d_linear_dgrad_f16x2(bad, bad, bad, 4, 64, 64, bad, 0, z, 0, bad, sz, z) == EINVAL
    assert L.m3d_linear_dgrad_f16x2(bad, bad, bad, 4, 64, 64, z, 0, bad, 1025, bad, sz, z) == EINVAL
    assert L.m3d_linear_wgrad_f16x2(bad, bad, bad, z, 4, 64, 64, bad, 0, z, 0, bad, sz, z) == EINVAL
    assert L.m3d_linear_dgrad_f16x2(C.c_void_p(18), bad, bad, 4, 64, 64, z, 0, z, 0, bad, sz, z) == EINVAL
    assert L.m3d_linear_dgrad_f16x2(C.c_void_p(20), bad, bad, 4, 64, 64, z, 0, z, 0, bad, sz, z) == EUNSUPPORTED
    assert L.m3d_linear_wgrad_f16x2(bad, C.c_void_p(20), bad, z, 4, 64, 64, z, 0, z, 0, bad, sz, z) == EUNSUPPORTED
    assert L.m3d_linear_dgrad_f16x2(bad, bad, bad, 4, 64, 64, z, 0, z, 0, bad, C.c_size_t(255), z) == EINVAL
    assert L.m3d_linear_wgrad_f16x2(bad, bad, bad, z, 4, 64, 64, z, 0, z, 0, bad, C.c_size_t(255), z) == EINVAL


# ------------------------------------------------------------------ the planner
def test_planner_routes_only_supported_shapes_at_or_above_min_work(L):
    from m3d import conv_plan as cp
    assert cp.LINEAR_BACKWARD_F16X2_MIN_WORK > 0
    for M, N, K in LC.CASES + SWEEP + [(128, 1024, 87808), (256, 1024, 43904), (64, 1024, 87808), (512, 1024, 87808), (256, 1024, 1024)]:
        assert cp.linear_backward_kernel(M, N, K, "fp32") == "fp32"
        assert cp.linear_backward_kernel(M, N, K, "fp32", min_work=0) == "fp32"
        ok = supported_rule(M, N, K)
        assert cp.linear_backward_kernel(M, N, K, "f16x2", min_work=0) == ("f16x2" if ok else "fp32"), (M, N, K)
        want = "f16x2" if ok and M * N * K >= cp.LINEAR_BACKWARD_F16X2_MIN_WORK else "fp32"
        assert cp.linear_backward_kernel(M, N, K, "f16x2") == want, (M, N, K)
        assert cp.linear_backward_kernel(M, N, K, "f16x2", min_work=M * N * K + 1) == "fp32"
    with pytest.raises(ValueError):
        cp.linear_backward_kernel(4, 64, 64, "bf16")


def test_switch_defaults_to_fp32_and_install_leaves_it():
    import m3d.compat as compat
    assert compat.get_linear_backward() == "fp32"
    prev = compat.set_linear_backward("f16x2", min_work=0)
    try:
        assert prev == "fp32" and compat.get_linear_backward() == "f16x2"
        with pytest.raises(ValueError):
            compat.set_linear_backward("f16")
        with pytest.raises(ValueError):
            compat.set_linear_backward("f16x2", min_work=-1)
    finally:
        compat.set_linear_backward("fp32")
    assert compat.get_linear_backward() == "fp32"
