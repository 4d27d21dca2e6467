"""CPU: the Adam solver and the gradient clip (csrc/adam.hip, m3d/solver.py) without a GPU.  The NumPy restatement of the update meets
its derived bounds against fp64, and so does what the installed torch.optim.Adam did from the same state (tests/golden/adam.npz, written
by tests/golden/gen_adam.py); the clip coefficient follows the reference's recorded clip_gradient; m3d.Solver(TYPE="Adam") reproduces
the rates the reference's update_learning_rate gave a torch.optim.Adam, with no momentum correction; state dicts pass to
torch.optim.Adam and back; the C ABI validates."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import adam_reference as AR
import sgd_reference as SR


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("adam")


# ---------------------------------------------------------------------------------------------------------------- 1. restatement
@pytest.mark.parametrize("case", list(AR.STEP_CASES))
def test_restatement_and_torch_meet_the_bounds(case, fixture):
    a = AR.load_case(fixture, case)
    n, lr, wd, t, betas, eps = AR.STEP_CASES[case]
    p, g, m, v = a["p"], a["g"], a["m"], a["v"]
    assert p.size == n and (g == 0).any() and ((g == 0) & (v == 0)).any()
    mine = AR.step(p, g, m, v, lr, wd, t, betas, eps)
    wr = AR.check_step(p, g, m, v, lr, wd, t, betas, eps, None, *mine, what="restatement")
    wt = AR.check_step(p, g, m, v, lr, wd, t, betas, eps, None, a["p_new"], a["m_new"], a["v_new"], what="torch")
    print("%s: largest error / bound (p', m', v'): restatement %.3f %.3f %.3f, torch %.3f %.3f %.3f" % ((case,) + wr + wt))
    if lr != 0:
        assert max(wr) > 0.05, "the bounds are not vacuous"


@pytest.mark.parametrize("s", [0.25, 0.0707734301686287, 1.0])
def test_restatement_with_a_coefficient_meets_the_bounds(s, fixture):
    a = AR.load_case(fixture, "second")
    n, lr, wd, t, betas, eps = AR.STEP_CASES["second"]
    args = (a["p"], a["g"], a["m"], a["v"], lr, wd, t, betas, eps, s)
    AR.check_step(*args, *AR.step(*args), what="restatement, s = %r" % s)
    if s == 1.0:       # a coefficient of 1 is exact
        for x, y in zip(AR.step(*args), AR.step(*args[:-1])):
            assert np.array_equal(AR.bits(x), AR.bits(y))


def test_zero_gradient_and_zero_second_moment(fixture):
    """g = 0, v = 0, wd = 0: q = eps, p' = p - lr_step (m' / eps) with m' = m + o1 (0 - m); at lr = 0 the parameter stays exactly"""
    a = AR.load_case(fixture, "late")
    n, lr, wd, t, betas, eps = AR.STEP_CASES["late"]
    blk = (a["g"] == 0) & (a["v"] == 0)
    p, g, m, v = (a[k][blk] for k in "pgmv")
    p2, m2, v2 = AR.step(p, g, m, v, 0.0, 0.0, t, betas, eps)
    o1 = np.float32(1 - betas[0])
    assert np.array_equal(AR.bits(p2), AR.bits(p)) and not v2.any()
    assert np.array_equal(AR.bits(m2), AR.bits(m + o1 * (np.float32(0) - m)))


# ---------------------------------------------------------------------------------------------------------------- 2. clip
@pytest.mark.parametrize("case", list(AR.CLIP_CASES))
def test_clip_coefficient_follows_the_reference(case, fixture):
    a = AR.load_case(fixture, case)
    scale, clip_norm = AR.CLIP_CASES[case]
    names = [nm for nm, _ in AR.CLIP_MODEL] + ["unit"]
    grads = [a["grad." + nm] for nm in names]
    gsq, bad = AR.grad_stats(grads)
    exact = sum(float((g.astype(np.float64) ** 2).sum()) for g in grads)
    N = sum(g.size for g in grads)
    assert bad == 0 and abs(gsq - exact) <= N * 2.0 ** -53 * exact
    coef = AR.clip_coef(gsq, clip_norm)
    assert coef.dtype == np.float32
    if math.sqrt(gsq) <= clip_norm:
        assert coef == np.float32(1.0) and float(a["coef"]) == 1.0
    else:
        # The reference rounds in fp32 where this contract works in fp64: each parameter's norm (a sum of n squares: relative error at
        # most n u / 2 after the root, plus u for the root), its square (u), the sum of K such terms (K u), the root of the sum (halves
        # what is under it, plus u), the quotient (u); the coefficient here is rounded to fp32 once (u).
        n_max, K = max(g.size for g in grads), len(grads)
        bound = AR.U * ((n_max + 2 + 2 + K) / 2 + 3)
        rel = abs(float(coef) - float(a["coef"])) / float(a["coef"])
        print("%s: coefficient %.9g, the reference's %.9g, relative difference %.3g (bound %.3g)" % (case, coef, a["coef"], rel, bound))
        assert coef < 1.0 and rel <= bound
    # at the threshold and on either side of it
    assert AR.clip_coef(4.0, 2.0) == np.float32(1.0) and AR.clip_coef(3.999, 2.0) == np.float32(1.0) and AR.clip_coef(4.001, 2.0) < 1.0
    assert np.isnan(AR.clip_coef(np.nan, 2.0)) and AR.clip_coef(np.inf, 2.0) == 0.0


def test_grad_stats_order_depends_on_the_residue():
    """the restated tree is a function of the sizes, the order, the values and the residues; a sum of 8192 + 5 squares meets N 2^-53"""
    rng = np.random.RandomState(3)
    g = [(rng.standard_normal(n) * 3).astype(np.float32) for n in (AR.CHUNK + 5, 7, 0, 1)]
    exact = sum(float((x.astype(np.float64) ** 2).sum()) for x in g)
    for res in ([0, 0, 0, 0], [1, 2, 3, 0], [3, 3, 3, 3]):
        s, bad = AR.grad_stats(g, res)
        assert bad == 0 and abs(s - exact) <= sum(x.size for x in g) * 2.0 ** -53 * exact
    g[1][3] = np.inf
    g[0][AR.CHUNK + 1] = np.nan
    s, bad = AR.grad_stats(g)
    assert bad == 2 and np.isnan(s)


# ---------------------------------------------------------------------------------------------------------------- 3. Solver
def tiny_model(dtype=torch.float32, seed=None):
    out = []
    gen = None if seed is None else torch.Generator().manual_seed(seed)
    for name, shape in SR.MODEL:
        v = torch.zeros(shape, dtype=dtype) if gen is None else torch.randn(shape, generator=gen, dtype=dtype)
        out.append((name, torch.nn.Parameter(v)))
    return out


def test_cfg_accepts_adam_and_clip():
    import m3d
    c = m3d.SolverCfg(TYPE="Adam")
    assert (c.TYPE, c.BETAS, c.EPS, c.CLIP_NORM) == ("Adam", (0.9, 0.999), 1e-8, None)
    c = m3d.SolverCfg(TYPE="Adam", BETAS=[0.8, 0.99], EPS=1e-6, CLIP_NORM=5.0, **m3d.SolverCfg.SOMA)
    assert (c.BETAS, c.EPS, c.CLIP_NORM, c.STEPS, c.MAX_ITER) == ((0.8, 0.99), 1e-6, 5.0, m3d.SolverCfg.soma().STEPS, 9000)
    assert m3d.SolverCfg.nuclei(CLIP_NORM=1.0).TYPE == "SGD" and m3d.SolverCfg.soma(TYPE="SGD", CLIP_NORM=1.0).CLIP_NORM == 1.0
    for preset in (m3d.SolverCfg.nuclei, m3d.SolverCfg.soma):      # the shipped YAML files are SGD runs and go on refusing another TYPE
        with pytest.raises(ValueError):
            preset(TYPE="Adam")
    for bad in (dict(TYPE="AdamW"), dict(TYPE="adam"), dict(TYPE="Adam", BETAS=(0.9, 1.0)), dict(TYPE="Adam", EPS=0.0), dict(CLIP_NORM=0.0),
                dict(CLIP_NORM=float("inf")), dict(CLIP_NORM=-1.0)):
        with pytest.raises(ValueError):
            m3d.SolverCfg(**bad)
    s = m3d.Solver(tiny_model(), m3d.SolverCfg(TYPE="Adam", CLIP_NORM=2.0))
    assert s.adam and s.grad_sq is not None and s.nonfinite is not None and s.clip_coef is not None and float(s.clip_coef) == 1.0
    assert s.clip_coef.dtype == torch.float32 and s.clip_coef.dim() == 0
    plain = m3d.Solver(tiny_model(), m3d.SolverCfg())
    assert not plain.adam and plain.grad_sq is None and plain.clip_coef is None
    # the group keys are this torch's
    twin = torch.optim.Adam([torch.zeros(1)], lr=0.0).state_dict()["param_groups"][0]
    for g in s.param_groups:
        assert set(g) == set(twin) and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8
        assert not (g["amsgrad"] or g["maximize"] or g["decoupled_weight_decay"])
    assert [len(g["params"]) for g in s.param_groups] == [2, 2, 0]
    assert all(b.data_ptr() % 16 == 0 for b in s._bufs + s._bufs2)
    assert not set(b.data_ptr() for b in s._bufs) & set(b.data_ptr() for b in s._bufs2)


@pytest.mark.parametrize("case", AR.SCHEDULE_CASES)
def test_schedule_reproduces_the_reference(case, fixture):
    import m3d
    a = AR.load_case(fixture, "schedule_" + case)
    assert int(a["corrections"]) == 0
    cfg = AR.adam_cfg(case)
    solver = m3d.Solver(tiny_model(), cfg)
    rates = []
    for step in range(cfg.MAX_ITER):
        lr = solver.begin_step(step)
        assert lr == solver.lr == solver.param_groups[0]["lr"]
        assert solver.mscale == 1.0, "no momentum correction is ever pending under Adam (step %d)" % step
        rates.append((solver.param_groups[0]["lr"], solver.param_groups[1]["lr"]))
    rates = np.array(rates, np.float64)
    assert rates.shape == a["rates"].shape
    assert np.array_equal(rates, a["rates"]), "first difference at step %d" % int(np.argmax((rates != a["rates"]).any(1)))
    # the same keys under SGD do correct the momentum: the case would notice a solver that ignores TYPE
    sgd = m3d.Solver(tiny_model(), SR.solver_cfg(case))
    pending = []
    for step in range(cfg.MAX_ITER):
        sgd.begin_step(step)
        pending.append(sgd.mscale != 1.0)
        sgd.mscale = 1.0
    assert any(pending)


# ---------------------------------------------------------------------------------------------------------------- 4. state dicts
def torch_twin(solver, kind=torch.optim.Adam, **kw):
    return kind([dict(params=g["params"], lr=g["lr"], weight_decay=g["weight_decay"]) for g in solver.param_groups], **kw)


def test_state_dicts_pass_to_torch_and_back():
    import m3d
    named = tiny_model(seed=4)
    cfg = AR.adam_cfg("short_linear", BETAS=(0.8, 0.99), EPS=1e-6)
    solver = m3d.Solver(named, cfg)
    sd = solver.state_dict()
    assert sd["state"] == {} and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3], []]
    twin = torch_twin(solver, betas=(0.8, 0.99), eps=1e-6)
    twin.load_state_dict(sd)                                       # before the first step: no state
    # torch steps; the last parameter (fc2.bias) never has a gradient, the first sits the second step out
    rng = np.random.RandomState(9)
    order = solver.param_groups[0]["params"] + solver.param_groups[1]["params"]
    for step in range(3):
        for i, q in enumerate(order):
            q.grad = None if (i == 3 or (i == 0 and step == 1)) else torch.from_numpy(rng.standard_normal(tuple(q.shape)).astype(np.float32))
        twin.param_groups[0]["lr"], twin.param_groups[1]["lr"] = 0.004, 0.008
        twin.step()
    tsd = twin.state_dict()
    assert sorted(tsd["state"]) == [0, 1, 2] and [float(tsd["state"][i]["step"]) for i in (0, 1, 2)] == [2.0, 3.0, 3.0]
    solver.load_state_dict(tsd)
    assert solver.lr == 0.004 and solver.param_groups[1]["lr"] == 0.008 and solver._steps == [2, 3, 3, 0]
    sd = solver.state_dict()
    assert [set(g) for g in sd["param_groups"]] == [set(g) for g in tsd["param_groups"]]
    for mine, theirs in zip(sd["param_groups"], tsd["param_groups"]):
        assert mine == theirs
    assert sorted(sd["state"]) == [0, 1, 2]
    for i in range(3):
        mine, theirs = sd["state"][i], tsd["state"][i]
        assert list(mine) == list(theirs) == ["step", "exp_avg", "exp_avg_sq"]
        assert mine["step"].dtype == theirs["step"].dtype == torch.float32 and mine["step"].dim() == 0
        assert float(mine["step"]) == float(theirs["step"])
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(mine[k], theirs[k]) and mine[k].shape == order[i].shape
    # and back into torch, which goes on from there
    back = torch_twin(solver, betas=(0.8, 0.99), eps=1e-6)
    back.load_state_dict(sd)
    for i, q in enumerate(order[:3]):
        assert float(back.state[q]["step"]) == float(tsd["state"][i]["step"])
        assert torch.equal(back.state[q]["exp_avg"], tsd["state"][i]["exp_avg"])
        assert torch.equal(back.state[q]["exp_avg_sq"], tsd["state"][i]["exp_avg_sq"])
    assert order[3] not in back.state
    # what this solver does not build is refused
    for key in ("amsgrad", "maximize", "decoupled_weight_decay"):
        bad = {"state": tsd["state"], "param_groups": [dict(g) for g in tsd["param_groups"]]}
        bad["param_groups"][1][key] = True
        with pytest.raises(ValueError):
            solver.load_state_dict(bad)
    with pytest.raises(ValueError):
        solver.load_state_dict({"state": {}, "param_groups": tsd["param_groups"][:2]})
    # state missing from a saved dict loads as zeros and step 0
    solver.load_state_dict({"state": {1: tsd["state"][1]}, "param_groups": tsd["param_groups"]})
    assert sorted(solver.state_dict()["state"]) == [1] and solver._steps == [0, 3, 0, 0]
    assert all(float(b.abs().max()) == 0 for i, b in enumerate(solver._bufs + solver._bufs2) if i % 4 != 1)


def test_wrong_type_state_raises():
    import m3d
    adam = m3d.Solver(tiny_model(), AR.adam_cfg("short_linear"))
    sgd = m3d.Solver(tiny_model(), SR.solver_cfg("short_linear"))
    with pytest.raises(ValueError):
        adam.load_state_dict(sgd.state_dict())
    with pytest.raises(ValueError):
        sgd.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError):
        adam.load_state_dict(torch_twin(sgd, torch.optim.SGD, momentum=0.9).state_dict())
    with pytest.raises(ValueError):
        sgd.load_state_dict(torch_twin(adam).state_dict())
    sgd.load_state_dict(torch_twin(sgd, torch.optim.SGD, momentum=0.9).state_dict())
    adam.load_state_dict(torch_twin(adam).state_dict())


def test_checkpoint_round_trip(tmp_path):
    import m3d

    def model():
        m = torch.nn.Sequential()
        m.add_module("fc1", torch.nn.Linear(5, 4))
        m.add_module("fc2", torch.nn.Linear(2, 5))
        return m
    cfg = AR.adam_cfg("short_linear", CLIP_NORM=1.0)
    m1, m2 = model(), model()
    s1, s2 = m3d.Solver(m1.named_parameters(), cfg), m3d.Solver(m2.named_parameters(), cfg)
    for step in range(10):
        s1.begin_step(step)
    state = {i: {"step": torch.tensor(float(3 + i)), "exp_avg": torch.randn(shape), "exp_avg_sq": torch.rand(shape)}
             for i, shape in ((0, (4, 5)), (1, (5, 2)), (3, (5,)))}
    s1.load_state_dict({"state": state, "param_groups": s1.state_dict()["param_groups"]})
    path = m3d.save_ckpt(str(tmp_path), 9, m1, s1)
    assert m3d.load_ckpt(path, m2, s2) == 10
    a, b = s1.state_dict(), s2.state_dict()
    assert a["param_groups"] == b["param_groups"] and sorted(a["state"]) == sorted(b["state"]) == [0, 1, 3]
    for i in (0, 1, 3):
        assert float(b["state"][i]["step"]) == 3 + i
        assert torch.equal(a["state"][i]["exp_avg"], b["state"][i]["exp_avg"]) and torch.equal(a["state"][i]["exp_avg_sq"], b["state"][i]["exp_avg_sq"])
    assert s2.lr == s1.lr and s2.k == s1.k == 2 and s2._steps == [3, 4, 0, 6]


# ---------------------------------------------------------------------------------------------------------------- 5. ABI
EINVAL, EUNSUPPORTED = -1, -4
OK4 = (0x10000, 0x20000, 0x30000, 0x40000)


def adam_call(L, tensors, count, beta1=0.9, beta2=0.999, eps=1e-8, gscale=None, stats=None, bc2=0.5):
    from m3d._lib import AdamTensor
    arr = (AdamTensor * max(len(tensors), 1))()
    for e, (p, g, m, v, n) in zip(arr, tensors):
        e.p, e.g, e.m, e.v, e.n, e.lr_step, e.bc2_sqrt, e.wd = p, g, m, v, n, 0.01, bc2, 0.0
    return L.m3d_adam_step(arr if tensors else None, count, C.c_double(beta1), C.c_double(beta2), C.c_double(eps), gscale, stats, None, None, None)


def clip_call(L, tensors, count, clip_norm=1.0, stats=0x1000, coef=0x2000, ws=None, nbytes=None):
    from m3d._lib import GradTensor
    arr = (GradTensor * max(len(tensors), 1))()
    for e, (g, n) in zip(arr, tensors):
        e.g, e.n = g, n
    return L.m3d_grad_clip_coef(arr if tensors else None, count, C.c_double(clip_norm), C.c_void_p(stats), C.c_void_p(coef), ws, nbytes, None)


def scaled_call(L, tensors, count, gscale=None, momentum=0.9):
    from m3d._lib import SgdTensor
    arr = (SgdTensor * max(len(tensors), 1))()
    for e, (p, g, m, n) in zip(arr, tensors):
        e.p, e.g, e.m, e.n, e.lr, e.wd = p, g, m, n, 0.01, 0.0
    return L.m3d_sgd_step_scaled(arr if tensors else None, count, C.c_float(momentum), C.c_float(1.0), gscale, None, None, None, None)


def test_symbols(L):
    from m3d._lib import SYMBOLS
    import m3d
    for s in ("m3d_adam_step", "m3d_grad_clip_coef", "m3d_sgd_step_scaled"):
        assert s in SYMBOLS and hasattr(L, s), s
    for f in ("adam_step", "grad_clip_coef", "sgd_step_scaled"):
        assert callable(getattr(m3d, f))


def test_adam_limits_without_a_gpu(L):
    ok = OK4 + (64,)
    assert adam_call(L, [], -1) == EINVAL                                                  # count < 0
    assert adam_call(L, [OK4 + (-1,)], 1) == EINVAL                                        # n < 0
    for k in range(4):                                                                     # a NULL or misaligned pointer
        for bad in (None, OK4[k] + 2, OK4[k] + 1):
            ptrs = list(OK4)
            ptrs[k] = bad
            assert adam_call(L, [ok, tuple(ptrs) + (64,)], 2) == EINVAL, (k, bad)
    for i in range(4):                                                                     # any two of p, g, m, v overlap
        for j in range(4):
            if i != j:
                ptrs = list(OK4)
                ptrs[i] = OK4[j] + 0xfc                                                    # by one element (64 floats = 256 bytes)
                assert adam_call(L, [tuple(ptrs) + (64,)], 1) == EINVAL, (i, j)
    for b in (-0.1, 1.0, 1.5, float("nan")):                                               # betas outside [0, 1)
        assert adam_call(L, [ok], 1, beta1=b) == EINVAL and adam_call(L, [ok], 1, beta2=b) == EINVAL
    for e in (0.0, -1e-8, 1e-60, float("nan")):                                            # eps not positive (as fp32)
        assert adam_call(L, [ok], 1, eps=e) == EINVAL
    for b in (0.0, -0.5, 1.0000001, float("nan")):                                         # bc2_sqrt outside (0, 1]
        assert adam_call(L, [ok], 1, bc2=b) == EINVAL
    assert adam_call(L, [ok], 1, gscale=C.c_void_p(0x5002)) == EINVAL                      # a misaligned coefficient pointer
    assert adam_call(L, [], 65537) == EUNSUPPORTED                                         # count > 65536
    assert adam_call(L, [OK4 + (1 << 40,)], 1) == EUNSUPPORTED                             # n >= 2^40
    # legal and nothing to do: no pointer is followed, nothing is launched
    assert adam_call(L, [], 0) == 0
    assert adam_call(L, [(None, None, None, None, 0), (0x10001, 0x10001, 0x10001, 0x10001, 0)], 2, bc2=0.0) == 0
    assert adam_call(L, [(None, None, None, None, 0)], 1, beta1=0.0, beta2=0.0, bc2=1.0) == 0
    # the size query: 16 bytes per chunk with statistics, nothing without
    from m3d._lib import AdamTensor
    chunk = L.m3d_sgd_chunk()
    arr = (AdamTensor * 2)()
    for e, n in zip(arr, (chunk + 1, 3)):
        e.p, e.g, e.m, e.v, e.n, e.bc2_sqrt = 0x10000000, 0x20000000, 0x30000000, 0x40000000, n, 1.0
    need = C.c_size_t(99)
    b1, b2, ep = C.c_double(0.9), C.c_double(0.999), C.c_double(1e-8)
    assert L.m3d_adam_step(arr, 2, b1, b2, ep, None, C.c_void_p(0x1000), None, C.byref(need), None) == 0 and need.value == 48
    assert L.m3d_adam_step(arr, 2, b1, b2, ep, None, None, None, C.byref(need), None) == 0 and need.value == 0
    assert L.m3d_adam_step(arr, 2, b1, b2, ep, None, C.c_void_p(0x1004), C.c_void_p(0x2000), C.byref(need), None) == EINVAL


def test_clip_limits_without_a_gpu(L):
    ok = (0x20000, 64)
    assert clip_call(L, [], -1) == EINVAL
    assert clip_call(L, [(0x20000, -1)], 1) == EINVAL
    assert clip_call(L, [ok, (None, 64)], 2) == EINVAL and clip_call(L, [ok, (0x20002, 64)], 2) == EINVAL
    for c in (0.0, -1.0, float("inf"), float("nan")):                                      # clip_norm not positive and finite
        assert clip_call(L, [ok], 1, clip_norm=c) == EINVAL
    assert clip_call(L, [ok], 1, stats=0) == EINVAL and clip_call(L, [ok], 1, coef=0) == EINVAL
    assert clip_call(L, [ok], 1, coef=0x2002) == EINVAL
    assert clip_call(L, [ok], 1, stats=0x1004, ws=C.c_void_p(0x3000), nbytes=C.byref(C.c_size_t(1 << 20))) == EINVAL
    assert clip_call(L, [], 65537) == EUNSUPPORTED and clip_call(L, [(0x20000, 1 << 40)], 1) == EUNSUPPORTED
    need = C.c_size_t(99)
    chunk = L.m3d_sgd_chunk()
    assert clip_call(L, [(0x20000000, 2 * chunk + 1), (None, 0), (0x30000000, 1)], 3, nbytes=C.byref(need)) == 0 and need.value == 64
    small = C.c_size_t(63)
    assert clip_call(L, [(0x20000000, 2 * chunk + 1), (0x30000000, 1)], 2, ws=C.c_void_p(0x3000), nbytes=C.byref(small)) == -3   # M3D_EWORKSPACE


def test_scaled_sgd_limits_without_a_gpu(L):
    ok = (0x10000, 0x20000, 0x30000, 64)
    assert scaled_call(L, [], -1) == EINVAL
    assert scaled_call(L, [ok, (0x10000, 0x20000, None, 64)], 2) == EINVAL                 # no buffer with momentum != 0
    assert scaled_call(L, [(0x10000, 0x10080, 0x30000, 64)], 1) == EINVAL                  # p and g overlap
    assert scaled_call(L, [ok], 1, gscale=C.c_void_p(0x5001)) == EINVAL                    # a misaligned coefficient pointer
    assert scaled_call(L, [], 65537) == EUNSUPPORTED
    assert scaled_call(L, [], 0) == 0 and scaled_call(L, [(None, None, None, 0)], 1, gscale=C.c_void_p(0x5000)) == 0


def test_no_cpu_path(L):
    import m3d
    t = [torch.zeros(8) for _ in range(4)]
    with pytest.raises(m3d.M3DError):
        m3d.adam_step([t[0]], [t[1]], [t[2]], [t[3]], [0.01], [0.0], [1], (0.9, 0.999), 1e-8)
    with pytest.raises(m3d.M3DError):
        m3d.sgd_step_scaled([t[0]], [t[1]], [t[2]], [0.01], [0.0], 0.9)
    with pytest.raises(m3d.M3DError):
        m3d.grad_clip_coef([t[1]], 1.0, torch.zeros(2, dtype=torch.float64), torch.zeros(1))
    with pytest.raises(m3d.M3DError):
        m3d.adam_step([t[0]], [t[1]], [t[2]], [], [0.01], [0.0], [1], (0.9, 0.999), 1e-8)
    lin = torch.nn.Linear(3, 2)
    solver = m3d.Solver(lin.named_parameters(), m3d.SolverCfg(TYPE="Adam", CLIP_NORM=1.0))
    solver.begin_step(0)
    for q in lin.parameters():
        q.grad = torch.ones_like(q)
    with pytest.raises(m3d.M3DError):
        solver.step()
    assert solver._steps == [0, 0] and solver.state_dict()["state"] == {}
