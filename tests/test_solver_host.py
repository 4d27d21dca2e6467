"""CPU: the solver (csrc/sgd.hip, m3d/solver.py) without a GPU.  The NumPy restatement of the update meets the derived
bounds against fp64, and torch.optim.SGD on the CPU lies within the same bounds; m3d.Solver reproduces the reference's recorded rates and
momentum corrections (tests/golden/solver.npz, written by tests/golden/gen_solver.py from the reference's own update_learning_rate) with
==; the restatement under that schedule follows the reference's fp64 trajectories as closely as torch's own fp32 SGD does; state dicts
pass to torch.optim.SGD and back; checkpoints round-trip; the C ABI validates."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sgd_reference as SR


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


@pytest.fixture(scope="module")
def fixture(golden):
    return golden("solver")


def tiny_model(arrays=None, dtype=torch.float32):
    """the fixture's model as named CPU parameters (its recorded initial values, or zeros)"""
    out = []
    for name, shape in SR.MODEL:
        v = torch.zeros(shape, dtype=dtype) if arrays is None else torch.tensor(arrays["init." + name], dtype=dtype)
        out.append((name, torch.nn.Parameter(v)))
    return out


# ---------------------------------------------------------------------------------------------------------------- 1. restatement
def magnitudes(rng, n):
    """signed values with magnitudes 2^[-20, 8]: no product of the update is subnormal"""
    return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-20, 8, n)).astype(np.float32)


STEP_CASES = [  # lr, wd, momentum, mscale, with a buffer
    (0.01, 1e-4, 0.9, 1.0, True), (0.02, 0.0, 0.9, 1.0, True), (0.005, 1e-4, 0.9, 0.5, True), (0.0033, 5e-4, 0.5, 1.4, True),
    (0.01, 1e-4, 0.0, 1.0, False), (0.01, 0.0, 0.0, 1.0, False), (1.0, 0.0, 0.0, 1.0, True),
]


@pytest.mark.parametrize("lr,wd,mu,ms,has_m", STEP_CASES)
def test_restatement_meets_the_bounds(lr, wd, mu, ms, has_m):
    rng = np.random.RandomState(7)
    n = 100003
    p, g = magnitudes(rng, n), magnitudes(rng, n)
    m = magnitudes(rng, n) if has_m else None
    p2, m2 = SR.step(p, g, m, lr, wd, mu, ms)
    wp, wm = SR.check_step(p, g, m, lr, wd, mu, ms, p2, m2, "restatement")
    print("restatement: largest error / bound: p' %.3f m' %.3f" % (wp, wm))
    assert wp > 0.05, "the bound is not vacuous"
    # torch.optim.SGD in fp32 on the same state: other roundings (FMA), the same bounds
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.SGD([tp], lr=lr, momentum=mu, weight_decay=wd)
    if has_m and mu != 0:
        opt.state[tp]["momentum_buffer"] = torch.from_numpy(m.copy()) * ms       # _CorrectMomentum's own multiplication
    tp.grad = torch.from_numpy(g.copy())
    opt.step()
    tm = opt.state[tp]["momentum_buffer"].numpy() if (has_m and mu != 0) else None
    if has_m and mu == 0:       # torch keeps no buffer without momentum: the contract's m' = 0 c + d = d there
        SR.check_step(p, g, None, lr, wd, mu, ms, tp.detach().numpy(), None, "torch")
    else:
        SR.check_step(p, g, m, lr, wd, mu, ms, tp.detach().numpy(), tm, "torch")


def test_first_step_is_buf_equals_grad():
    """a zero-filled buffer reproduces torch's first step (buf = d), and mscale == 1 is exact"""
    rng = np.random.RandomState(8)
    p, g = magnitudes(rng, 1000), magnitudes(rng, 1000)
    p2, m2 = SR.step(p, g, np.zeros_like(p), 0.01, 1e-4, 0.9, 1.0)
    d = g + np.float32(1e-4) * p
    assert np.array_equal(SR.bits(m2), SR.bits(d)) and np.array_equal(SR.bits(p2), SR.bits(p - np.float32(0.01) * d))


# ---------------------------------------------------------------------------------------------------------------- 2. schedule
def drive(case, arrays, on_step=None):
    """m3d.Solver on CPU parameters through every step of a case -> (rates [n,2], [(step, factor)]); a case with a resume step passes
    its state through state_dict() / load_state_dict() into a fresh Solver(start_step=...) there.  on_step(solver, step, factor) stands
    in for step(): the correction is handed over and reset as step() does."""
    import m3d
    cfg = SR.solver_cfg(case)
    resume_after = SR.CASES[case][2]
    solver = m3d.Solver(tiny_model(), cfg)
    rates, corrections = [], []
    for step in range(cfg.MAX_ITER):
        lr = solver.begin_step(step)
        assert lr == solver.lr == solver.param_groups[0]["lr"]
        rates.append((solver.param_groups[0]["lr"], solver.param_groups[1]["lr"]))
        if solver.mscale != 1.0:
            corrections.append((step, solver.mscale))
        if on_step:
            on_step(solver, step, solver.mscale)
        solver.mscale = 1.0
        if step == resume_after:
            fresh = m3d.Solver(tiny_model(), cfg, start_step=step + 1)
            fresh.load_state_dict(solver.state_dict())
            solver = fresh
    return np.array(rates, np.float64), corrections


@pytest.mark.parametrize("case", list(SR.CASES))
def test_schedule_reproduces_the_reference(case, fixture):
    a = SR.load_case(fixture, case)
    rates, corrections = drive(case, a)
    assert rates.shape == a["rates"].shape
    assert np.array_equal(rates, a["rates"]), "first difference at step %d" % int(np.argmax((rates != a["rates"]).any(1)))
    assert [s for s, _ in corrections] == a["correction_steps"].tolist()
    assert [f for _, f in corrections] == a["correction_factors"].tolist()
    # the restated schedule of sgd_reference says the same
    sch = SR.Schedule(SR.keys_of(case))
    resume_after = SR.CASES[case][2]
    for step in range(len(rates)):
        lr, lr_bias, f = sch.begin(step)
        assert (lr, lr_bias) == tuple(a["rates"][step])
        assert (f != 1.0) == (step in a["correction_steps"])
        if step == resume_after:
            sch = SR.Schedule(SR.keys_of(case), start_step=step + 1, lr=lr)


def test_cfg_refuses_what_is_not_built():
    import m3d
    with pytest.raises(ValueError):
        m3d.SolverCfg.nuclei(TYPE="Adam")
    with pytest.raises(ValueError):
        m3d.SolverCfg.soma(LR_POLICY="step")
    with pytest.raises(TypeError):
        m3d.SolverCfg.nuclei(BASE_LRR=1)
    c, s = m3d.SolverCfg.nuclei(), m3d.SolverCfg.soma(BASE_LR=0.02)
    assert (c.STEPS, c.MAX_ITER, s.STEPS, s.MAX_ITER, s.BASE_LR) == ((0, 3000, 6000, 9000, 12000), 12000, (0, 3000, 6000, 9000), 9000, 0.02)
    for k, v in SR.DEFAULT_KEYS.items():
        assert getattr(c, k) == v, k
    assert c.SNAPSHOT_ITERS == 3000


# ---------------------------------------------------------------------------------------------------------------- 3. trajectory
GROUP = {name: (1 if "bias" in name else 0) for name, _ in SR.MODEL}


def deviation(a, params):
    """largest |fp32 trajectory - fp64 golden| over all steps and parameters, relative to the largest parameter magnitude"""
    top = max(np.abs(a["p." + n]).max() for n, _ in SR.MODEL)
    return max(np.abs(np.stack(params[n]).astype(np.float64) - a["p." + n]).max() for n, _ in SR.MODEL) / top


@pytest.mark.parametrize("case", SR.SHORT_CASES)
def test_trajectory_follows_the_reference(case, fixture):
    a = SR.load_case(fixture, case)
    keys = SR.keys_of(case)
    wds = (keys["WEIGHT_DECAY"], keys["WEIGHT_DECAY"] if keys["BIAS_WEIGHT_DECAY"] else 0.0)
    # the restatement under m3d.Solver's schedule
    p = {n: a["init." + n].astype(np.float32) for n, _ in SR.MODEL}
    m = {n: np.zeros_like(p[n]) for n in p}
    mine = {n: [] for n in p}

    def on_step(solver, step, factor):
        for n in p:
            g = solver.param_groups[GROUP[n]]
            p[n], m[n] = SR.step(p[n], a["grad." + n][step], m[n], g["lr"], g["weight_decay"], g["momentum"], factor)
            mine[n].append(p[n])
    drive(case, a, on_step)
    # torch.optim.SGD in fp32 on the CPU with the same gradients, rates and corrections (the recorded ones)
    named = tiny_model(a)
    opt = torch.optim.SGD([dict(params=[q for n, q in named if GROUP[n] == i], lr=0.0, weight_decay=wds[i]) for i in (0, 1)],
                          momentum=keys["MOMENTUM"])
    theirs = {n: [] for n in p}
    factor_at = dict(zip(a["correction_steps"].tolist(), a["correction_factors"].tolist()))
    for step in range(keys["MAX_ITER"]):
        for i in (0, 1):
            opt.param_groups[i]["lr"] = float(a["rates"][step, i])
        if step in factor_at:
            for _, q in named:
                opt.state[q]["momentum_buffer"] *= factor_at[step]
        for n, q in named:
            q.grad = torch.from_numpy(a["grad." + n][step].copy())
        opt.step()
        for n, q in named:
            theirs[n].append(q.detach().numpy().copy())
    dev_mine, dev_torch = deviation(a, mine), deviation(a, theirs)
    print("%s: deviation from the fp64 trajectory, relative to the largest parameter: restatement %.3e, torch fp32 %.3e" % (
        case, dev_mine, dev_torch))
    assert dev_mine <= 4 * dev_torch


# ---------------------------------------------------------------------------------------------------------------- 4. state dicts
def torch_twin(solver):
    return torch.optim.SGD([dict(params=g["params"], lr=g["lr"], weight_decay=g["weight_decay"]) for g in solver.param_groups],
                           momentum=solver.param_groups[0]["momentum"])


def test_state_dicts_pass_to_torch_and_back(fixture):
    import m3d
    a = SR.load_case(fixture, "short_linear")
    named = tiny_model(a)
    solver = m3d.Solver(named, SR.solver_cfg("short_linear"))
    sd = solver.state_dict()
    assert sd["state"] == {} and [g["params"] for g in sd["param_groups"]] == [[0, 1], [2, 3], []]
    twin = torch_twin(solver)
    twin.load_state_dict(sd)                                       # before the first step: no buffers
    # a few torch steps, then into the solver
    for step in range(3):
        for n, q in named:
            q.grad = torch.from_numpy(a["grad." + n][step].copy())
        twin.param_groups[0]["lr"], twin.param_groups[1]["lr"] = 0.004, 0.008
        twin.step()
    tsd = twin.state_dict()
    solver.load_state_dict(tsd)
    assert solver.lr == 0.004 and solver.param_groups[1]["lr"] == 0.008
    sd = solver.state_dict()
    assert [set(g) for g in sd["param_groups"]] == [set(g) for g in tsd["param_groups"]]
    for mine, theirs in zip(sd["param_groups"], tsd["param_groups"]):
        assert mine == theirs
        assert (mine["dampening"], mine["nesterov"], mine["momentum"]) == (0, False, 0.9)
    assert sorted(sd["state"]) == sorted(tsd["state"]) == [0, 1, 2, 3]
    for i in range(4):
        assert torch.equal(sd["state"][i]["momentum_buffer"], tsd["state"][i]["momentum_buffer"])
        assert sd["state"][i]["momentum_buffer"].shape == solver.param_groups[i // 2]["params"][i % 2].shape
    # a pending correction is folded into the buffers that are saved
    solver.mscale = 0.5
    folded = solver.state_dict()
    for i in range(4):
        assert torch.equal(folded["state"][i]["momentum_buffer"], tsd["state"][i]["momentum_buffer"] * 0.5)
    solver.mscale = 1.0
    # and back into torch
    back = torch_twin(solver)
    back.load_state_dict(folded)
    for i, q in enumerate(solver.param_groups[0]["params"] + solver.param_groups[1]["params"]):
        assert torch.equal(back.state[q]["momentum_buffer"], folded["state"][i]["momentum_buffer"])
    # buffers missing from the saved state load as zeros
    partial = {"state": {0: tsd["state"][0]}, "param_groups": tsd["param_groups"]}
    solver.load_state_dict(partial)
    assert sorted(solver.state_dict()["state"]) == [0]
    assert all(float(b.abs().max()) == 0 for b in solver._bufs[1:])
    with pytest.raises(ValueError):
        solver.load_state_dict({"state": {}, "param_groups": tsd["param_groups"][:2]})


def test_momentum_views_are_16_byte_aligned():
    import m3d
    named = [("a.weight", torch.nn.Parameter(torch.zeros(5))), ("a.bias", torch.nn.Parameter(torch.zeros(3))),
             ("b.weight", torch.nn.Parameter(torch.zeros(2, 3))), ("frozen.weight", torch.nn.Parameter(torch.zeros(2), requires_grad=False))]
    s = m3d.Solver(named, m3d.SolverCfg.nuclei())
    assert [len(g["params"]) for g in s.param_groups] == [2, 1, 0]
    assert all(b.data_ptr() % 16 == 0 for b in s._bufs) and [b.numel() for b in s._bufs] == [5, 6, 3]
    assert (s.param_groups[0]["weight_decay"], s.param_groups[1]["weight_decay"], s.param_groups[2]["weight_decay"]) == (0.0001, 0, 0.0)


def test_checkpoint_round_trip(tmp_path, fixture):
    import m3d
    a = SR.load_case(fixture, "short_linear")
    model = torch.nn.Sequential()
    model.add_module("fc1", torch.nn.Linear(5, 4))
    model.add_module("fc2", torch.nn.Linear(2, 5))
    cfg = SR.solver_cfg("short_linear")
    solver = m3d.Solver(model.named_parameters(), cfg)
    for step in range(10):
        solver.begin_step(step)
        solver.mscale = 1.0
    buffers = {0: torch.randn(4, 5), 1: torch.randn(5, 2), 2: torch.randn(4), 3: torch.randn(5)}
    solver.load_state_dict({"state": {i: {"momentum_buffer": b} for i, b in buffers.items()}, "param_groups": solver.state_dict()["param_groups"]})
    path = m3d.save_ckpt(str(tmp_path), 9, model, solver, train_size=7, batch_size=2)
    assert path == os.path.join(str(tmp_path), "ckpt", "model_step9.pth") and os.path.exists(path)
    raw = torch.load(path, map_location="cpu")
    assert sorted(raw) == ["batch_size", "model", "optimizer", "step", "train_size"]
    assert (raw["step"], raw["train_size"], raw["batch_size"]) == (9, 7, 2)
    model2 = torch.nn.Sequential()
    model2.add_module("fc1", torch.nn.Linear(5, 4))
    model2.add_module("fc2", torch.nn.Linear(2, 5))
    solver2 = m3d.Solver(model2.named_parameters(), cfg)
    assert m3d.load_ckpt(path, model2, solver2) == 10
    for (n1, p1), (n2, p2) in zip(model.state_dict().items(), model2.state_dict().items()):
        assert n1 == n2 and torch.equal(p1, p2)
    assert solver2.lr == solver.lr == float(a["rates"][9, 0]) and solver2.k == 2 and solver2.start_step == 10
    s1, s2 = solver.state_dict(), solver2.state_dict()
    assert s1["param_groups"] == s2["param_groups"]
    for i in range(4):
        assert torch.equal(s1["state"][i]["momentum_buffer"], s2["state"][i]["momentum_buffer"])
    # resumed, the schedule goes on as the reference's does
    for step in range(10, 20):
        solver2.begin_step(step)
        assert (solver2.param_groups[0]["lr"], solver2.param_groups[1]["lr"]) == tuple(a["rates"][step])
    model3 = torch.nn.Sequential()
    model3.add_module("fc1", torch.nn.Linear(5, 4))
    model3.add_module("fc2", torch.nn.Linear(2, 5))
    assert m3d.load_ckpt(path, model3) == 10                       # without a solver: the model alone


# ---------------------------------------------------------------------------------------------------------------- 5. ABI
def call(L, tensors, count, momentum=0.9, stats=None):
    from m3d._lib import SgdTensor
    arr = (SgdTensor * max(len(tensors), 1))()
    for e, (p, g, m, n) in zip(arr, tensors):
        e.p, e.g, e.m, e.n, e.lr, e.wd = p, g, m, n, 0.01, 0.0
    return L.m3d_sgd_step(arr if tensors else None, count, C.c_float(momentum), C.c_float(1.0), stats, None, None, None)


def test_abi_limits_without_a_gpu(L):
    from m3d._lib import SYMBOLS
    for s in ("m3d_sgd_step", "m3d_sgd_chunk"):
        assert s in SYMBOLS and hasattr(L, s), s
    assert L.m3d_sgd_chunk() >= 1024 and L.m3d_sgd_chunk() % 4 == 0
    EINVAL, EUNSUPPORTED = -1, -4
    ok = (0x10000, 0x20000, 0x30000, 64)
    assert call(L, [], -1) == EINVAL                                             # count < 0
    assert call(L, [(0x10000, 0x20000, 0x30000, -1)], 1) == EINVAL               # n < 0
    assert call(L, [ok, (0x10000, 0x20000, None, 64)], 2) == EINVAL              # no buffer with momentum != 0
    assert call(L, [(0x10000, 0x10080, 0x30000, 64)], 1) == EINVAL               # p and g overlap (64 floats = 256 bytes)
    assert call(L, [(0x10000, 0x20000, 0x200fc, 64)], 1) == EINVAL               # g and m overlap by one element
    assert call(L, [(0x10000, 0x20000, 0x0ff04, 64)], 1) == EINVAL               # m runs into p
    assert call(L, [(0x10002, 0x20000, 0x30000, 64)], 1) == EINVAL               # a pointer not 4-byte aligned
    assert call(L, [(0x10000, 0x20001, 0x30000, 64)], 1) == EINVAL
    assert call(L, [(0x10000, 0x20000, 0x30003, 64)], 1) == EINVAL
    assert call(L, [], 65537) == EUNSUPPORTED                                    # count > 65536
    assert call(L, [(0x10000, 0x20000, 0x30000, 1 << 40)], 1) == EUNSUPPORTED    # n >= 2^40
    # legal and nothing to do: no pointer is followed, nothing is launched
    assert call(L, [], 0) == 0
    assert call(L, [(None, None, None, 0), (0x10001, 0x10001, 0x10001, 0)], 2) == 0
    # the size query: 16 bytes per chunk with statistics, nothing without
    from m3d._lib import SgdTensor
    chunk = L.m3d_sgd_chunk()
    arr = (SgdTensor * 2)()
    for e, n in zip(arr, (chunk + 1, 3)):
        e.p, e.g, e.m, e.n = 0x10000000, 0x20000000, 0x30000000, n
    need = C.c_size_t(99)
    assert L.m3d_sgd_step(arr, 2, C.c_float(0.9), C.c_float(1.0), C.c_void_p(0x1000), None, C.byref(need), None) == 0 and need.value == 48
    assert L.m3d_sgd_step(arr, 2, C.c_float(0.9), C.c_float(1.0), None, None, C.byref(need), None) == 0 and need.value == 0


def test_no_cpu_path(L):
    import m3d
    p, g, m = torch.zeros(8), torch.zeros(8), torch.zeros(8)
    with pytest.raises(m3d.M3DError):
        m3d.sgd_step([p], [g], [m], [0.01], [0.0], 0.9)
    lin = torch.nn.Linear(3, 2)
    solver = m3d.Solver(lin.named_parameters(), m3d.SolverCfg.nuclei())
    solver.begin_step(0)
    for q in lin.parameters():
        q.grad = torch.ones_like(q)
    with pytest.raises(m3d.M3DError):
        solver.step()
    solver.zero_grad()
    assert all(q.grad is None for q in lin.parameters())
