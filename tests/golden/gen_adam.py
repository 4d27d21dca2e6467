"""Golden vectors for the Adam solver and the gradient clip: what the installed torch.optim.Adam (single-tensor path, CPU, fp32) does in
one step from a given state, what the REFERENCE's own `utils.net.clip_gradient` does to a tiny model's gradients, and what its
`utils.net.update_learning_rate` does to a torch.optim.Adam over short schedules under SOLVER.TYPE = 'Adam' (loaded through
oracle/ref_harness.py).  Writes tests/golden/adam.npz.

Single steps (adam_reference.STEP_CASES): p, g, m, v fp32 with |g| in 2^[-20, 4] and exact zeros, m = g-sized, v >= 0; the state is put
into the optimiser as torch keeps it (`step` = t - 1, `exp_avg`, `exp_avg_sq`), the gradient set, step() called; recorded: the inputs
and p', m', v'.
Clip (adam_reference.CLIP_CASES): the tiny model of adam_reference.CLIP_MODEL plus one 0-d parameter whose gradient is exactly 1, so
that its gradient after clip_gradient IS the coefficient the reference multiplied by; recorded: the gradients before and after.
Schedules (adam_reference.SCHEDULE_CASES): the loop of gen_solver.py around a torch.optim.Adam over the reference's three groups;
recorded: both group rates at every step and how often _CorrectMomentum ran (never: lib/utils/net.py:81 is for SGD).

Run in the build container only, after oracle/build_ref.sh:  python tests/golden/gen_adam.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import adam_reference as AR  # noqa: E402
import sgd_reference as SR  # noqa: E402
from gen_rpn_train import write  # noqa: E402
from gen_solver import YAML, decay_index  # noqa: E402


def step_inputs(rng, n):
    def mags(lo, hi):
        return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(lo, hi, n)).astype(np.float32)
    p, g, m = mags(-6, 3), mags(-20, 4), mags(-20, 4)
    v = (mags(-20, 4) ** 2).astype(np.float32)
    g[::17] = 0.0
    m[5::31], v[5::31] = 0.0, 0.0
    g[3::51], v[3::51] = 0.0, 0.0                 # g = 0 and v = 0: q = eps
    return p, g, m, v


def run_step(torch, name, seed):
    n, lr, wd, t, betas, eps = AR.STEP_CASES[name]
    p, g, m, v = step_inputs(np.random.RandomState(seed), n)
    tp = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([tp], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    if t > 1:
        opt.state[tp] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    else:                                          # torch's first step starts from zeros
        m, v = np.zeros_like(m), np.zeros_like(v)
    tp.grad = torch.from_numpy(g.copy())
    opt.step()
    st = opt.state[tp]
    assert float(st["step"]) == t
    return {"p": p, "g": g, "m": m, "v": v, "p_new": tp.detach().numpy().copy(), "m_new": st["exp_avg"].numpy().copy(),
            "v_new": st["exp_avg_sq"].numpy().copy()}


def run_clip(torch, net_utils, name, seed):
    scale, clip_norm = AR.CLIP_CASES[name]
    rng = np.random.RandomState(seed)
    model = torch.nn.Module()
    grads = {}
    for nm, shape in AR.CLIP_MODEL + (("unit", ()),):
        q = torch.nn.Parameter(torch.zeros(shape))
        model.register_parameter(nm.replace(".", "_"), q)
        grads[nm] = np.float32(1.0) if nm == "unit" else (rng.standard_normal(shape) * scale).astype(np.float32)
        q.grad = torch.tensor(grads[nm])
    net_utils.clip_gradient(model, clip_norm)
    out = {}
    for (nm, _), q in zip(AR.CLIP_MODEL + (("unit", ()),), model.parameters()):
        out["grad." + nm], out["clipped." + nm] = np.asarray(grads[nm], np.float32), q.grad.numpy().copy()
    out["coef"] = out["clipped.unit"].reshape(())
    return out


def run_schedule(H, torch, net_utils, name):
    """the loop of gen_solver.run_case (train_net_step.py:392-436) around torch.optim.Adam, no gradients: only the rates"""
    dataset, over, _, _ = SR.CASES[name]
    base = dict(WARM_UP_ITERS=500, WARM_UP_METHOD="linear")
    base.update(over)
    flat = ["SOLVER.TYPE", "Adam"]
    for k, v in base.items():
        flat += ["SOLVER." + k, list(v) if isinstance(v, tuple) else v]
    cfg = H.load_cfg(YAML[dataset], flat)
    S = cfg.SOLVER
    assert S.TYPE == "Adam"
    named = [(nm, torch.zeros(shape, requires_grad=True)) for nm, shape in SR.MODEL]
    nonbias = [p for n, p in named if "bias" not in n]
    bias = [p for n, p in named if "bias" in n]
    opt = torch.optim.Adam([{"params": nonbias, "lr": 0, "weight_decay": S.WEIGHT_DECAY},
                            {"params": bias, "lr": 0 * (S.BIAS_DOUBLE_LR + 1), "weight_decay": S.WEIGHT_DECAY if S.BIAS_WEIGHT_DECAY else 0},
                            {"params": [], "lr": 0, "weight_decay": S.WEIGHT_DECAY_GN}])
    calls = [0]
    original = net_utils._CorrectMomentum

    def counting(*a):
        calls[0] += 1
        original(*a)
    net_utils._CorrectMomentum = counting
    rates = np.zeros((S.MAX_ITER, 2), np.float64)
    try:
        lr, k = opt.param_groups[0]["lr"], decay_index(cfg, 0)
        for step in range(S.MAX_ITER):
            if step < S.WARM_UP_ITERS:
                if S.WARM_UP_METHOD == "constant":
                    factor = S.WARM_UP_FACTOR
                else:
                    alpha = step / S.WARM_UP_ITERS
                    factor = S.WARM_UP_FACTOR * (1 - alpha) + alpha
                net_utils.update_learning_rate(opt, lr, S.BASE_LR * factor)
                lr = opt.param_groups[0]["lr"]
            elif step == S.WARM_UP_ITERS:
                net_utils.update_learning_rate(opt, lr, S.BASE_LR)
                lr = opt.param_groups[0]["lr"]
            if k < len(S.STEPS) and step == S.STEPS[k]:
                net_utils.update_learning_rate(opt, lr, lr * S.GAMMA)
                lr = opt.param_groups[0]["lr"]
                k += 1
            rates[step] = opt.param_groups[0]["lr"], opt.param_groups[1]["lr"]
    finally:
        net_utils._CorrectMomentum = original
        H.load_cfg(YAML[dataset], ["SOLVER.TYPE", "SGD"])
    return {"rates": rates, "corrections": np.array(calls[0], np.int64)}


def build_arrays():
    import ref_harness as H
    H.install()
    import torch
    import utils.net as net_utils
    out = {}

    def put(name, arrays):
        for k, v in arrays.items():
            out[name + "/" + k] = v
    for i, name in enumerate(AR.STEP_CASES):
        put(name, run_step(torch, name, 70 + i))
    for i, name in enumerate(AR.CLIP_CASES):
        put(name, run_clip(torch, net_utils, name, 90 + i))
        print(name, "coefficient", float(out[name + "/coef"]))
    for name in AR.SCHEDULE_CASES:
        put("schedule_" + name, run_schedule(H, torch, net_utils, name))
    # ---- the properties the cases exist for
    assert float(out["clip_below/coef"]) == 1.0 and all(float(out[n + "/coef"]) < 1.0 for n in AR.CLIP_CASES if n != "clip_below")
    for name in AR.SCHEDULE_CASES:
        assert int(out["schedule_" + name + "/corrections"]) == 0, "no momentum correction under Adam"
        assert np.array_equal(out["schedule_" + name + "/rates"], np.load(os.path.join(HERE, "solver.npz"))[name + "/rates"]), \
            "the rates are those of the SGD run"
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "adam.npz")
    write(path, build_arrays())
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < 300 * 1024, "the fixture stays under 300 KB"
