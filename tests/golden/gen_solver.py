"""Golden vectors for the solver: drives torch.optim.SGD in fp64 with the REFERENCE's own `utils.net.update_learning_rate` (and through
it `_CorrectMomentum`) under the SOLVER keys of the two shipped yaml files, loaded through oracle/ref_harness.py, and writes
tests/golden/solver.npz.

The model is tiny (sgd_reference.MODEL: two weights and two biases, 40 values, fp64), grouped as tools/train_net_step.py:300-326 groups
a model; the gradients come from np.random.RandomState(seed), rounded to fp32.  The loop around the optimiser follows
train_net_step.py:392-436 and :474.  Recorded per case: both group rates at every step, the steps at which _CorrectMomentum ran and
its factor, and for the short cases the gradients, and parameters and buffers after every step.  `short_resume` saves a checkpoint
dictionary after step 10, builds a fresh model and optimiser, loads it and resumes at step 11 as train_net_step.py:336-356 does.

The generator asserts the properties the cases exist for.

Run in the build container only, after oracle/build_ref.sh:  python tests/golden/gen_solver.py"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import sgd_reference as SR  # noqa: E402
from gen_rpn_train import write  # noqa: E402

YAML = {"nuclei": "configs/cell_tracking_baseline/e2e_mask_rcnn_N3DH_SIM_dsn_body.yaml",
        "soma": "configs/soma_starting/e2e_mask_rcnn_soma_dsn_body.yaml"}
SEEDS = {name: 40 + i for i, name in enumerate(SR.CASES)}
SEEDS["short_resume"] = SEEDS["short_linear"]          # the same 20 steps


def make_model(torch, rng):
    return [(name, torch.tensor(rng.standard_normal(shape) * 0.5, dtype=torch.float64, requires_grad=True)) for name, shape in SR.MODEL]


def make_optimizer(torch, cfg, named):
    nonbias = [p for n, p in named if "bias" not in n]
    bias = [p for n, p in named if "bias" in n]
    groups = [{"params": nonbias, "lr": 0, "weight_decay": cfg.SOLVER.WEIGHT_DECAY},
              {"params": bias, "lr": 0 * (cfg.SOLVER.BIAS_DOUBLE_LR + 1),
               "weight_decay": cfg.SOLVER.WEIGHT_DECAY if cfg.SOLVER.BIAS_WEIGHT_DECAY else 0},
              {"params": [], "lr": 0, "weight_decay": cfg.SOLVER.WEIGHT_DECAY_GN}]
    return torch.optim.SGD(groups, momentum=cfg.SOLVER.MOMENTUM), nonbias + bias


def decay_index(cfg, start_step):
    for i in range(1, len(cfg.SOLVER.STEPS)):
        if cfg.SOLVER.STEPS[i] >= start_step:
            return i
    return len(cfg.SOLVER.STEPS)


def run_case(H, torch, net_utils, name):
    dataset, over, resume_after, full = SR.CASES[name]
    base = dict(WARM_UP_ITERS=500, WARM_UP_METHOD="linear")       # keys a case may change and the yaml does not reset
    base.update(over)
    flat = []
    for k, v in base.items():
        flat += ["SOLVER." + k, list(v) if isinstance(v, tuple) else v]
    cfg = H.load_cfg(YAML[dataset], flat)
    S = cfg.SOLVER
    keys = SR.keys_of(name)
    for k, v in keys.items():                                    # the restated defaults are the values the reference runs with
        got = getattr(S, k)
        assert (tuple(got) if isinstance(got, (list, tuple)) else got) == v, (name, k, got, v)
    assert S.TYPE == "SGD" and S.LR_POLICY == "steps_with_decay" and cfg.TRAIN.SNAPSHOT_ITERS == 3000
    rng = np.random.RandomState(SEEDS[name])
    named = make_model(torch, rng)
    opt, order = make_optimizer(torch, cfg, named)
    init = [p.detach().numpy().copy() for _, p in named]
    n = S.MAX_ITER
    grads = [rng.standard_normal((n,) + shape).astype(np.float32) for _, shape in SR.MODEL]
    corrections, now = [], [0]
    original = net_utils._CorrectMomentum

    def recording(optimizer, param_keys, correction):
        corrections.append((now[0], correction))
        original(optimizer, param_keys, correction)
    net_utils._CorrectMomentum = recording
    rates = np.zeros((n, 2), np.float64)
    traj_p = [np.zeros((n,) + shape, np.float64) for _, shape in SR.MODEL]
    traj_m = [np.zeros((n,) + shape, np.float64) for _, shape in SR.MODEL]
    try:
        lr = opt.param_groups[0]["lr"]
        k = decay_index(cfg, 0)
        step = 0
        while step < n:
            now[0] = step
            if step < S.WARM_UP_ITERS:
                if S.WARM_UP_METHOD == "constant":
                    factor = S.WARM_UP_FACTOR
                else:
                    assert S.WARM_UP_METHOD == "linear"
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
            opt.zero_grad()
            for (_, p), g in zip(named, grads):
                p.grad = torch.from_numpy(g[step].astype(np.float64))
            opt.step()
            rates[step] = opt.param_groups[0]["lr"], opt.param_groups[1]["lr"]
            if full:
                for i, (_, p) in enumerate(named):
                    traj_p[i][step] = p.detach().numpy()
                    traj_m[i][step] = opt.state[p]["momentum_buffer"].numpy()
            if resume_after is not None and step == resume_after:
                blob = io.BytesIO()
                torch.save({"step": step, "train_size": 0, "batch_size": 1, "model": {nm: p.detach() for nm, p in named},
                            "optimizer": opt.state_dict()}, blob)
                blob.seek(0)
                ckpt = torch.load(blob, map_location=lambda storage, loc: storage)
                named = make_model(torch, np.random.RandomState(999))       # a fresh model: everything must come from the checkpoint
                opt, order = make_optimizer(torch, cfg, named)
                with torch.no_grad():
                    for nm, p in named:
                        p.copy_(ckpt["model"][nm])
                opt.load_state_dict(ckpt["optimizer"])
                lr = opt.param_groups[0]["lr"]
                k = decay_index(cfg, ckpt["step"] + 1)
                resume_after = None
            step += 1
    finally:
        net_utils._CorrectMomentum = original
    out = {"rates": rates, "correction_steps": np.array([s for s, _ in corrections], np.int64),
           "correction_factors": np.array([f for _, f in corrections], np.float64), "seed": np.array(SEEDS[name], np.int64)}
    if full:
        for i, (nm, _) in enumerate(SR.MODEL):
            out["init." + nm], out["grad." + nm], out["p." + nm], out["m." + nm] = init[i], grads[i], traj_p[i], traj_m[i]
    return out, corrections


def build_arrays():
    import ref_harness as H
    H.install()
    import torch
    import utils.net as net_utils
    out = {}
    for name in SR.CASES:
        arrays, corrections = run_case(H, torch, net_utils, name)
        for k, v in arrays.items():
            out[name + "/" + k] = v
        print(name, "corrections", corrections[:8], "final rates", arrays["rates"][-1].tolist())
        # ---- the properties the cases exist for
        if SR.CASES[name][3]:
            assert len(corrections) >= 1, name + ": a short case contains a correction"
    assert out["nuclei_full/correction_factors"].tolist() == [0.5, 0.5, 0.5] and \
        out["nuclei_full/correction_steps"].tolist() == [3000, 6000, 9000]
    for k in ("p.", "m."):
        for nm, _ in SR.MODEL:
            assert np.array_equal(out["short_resume/" + k + nm], out["short_linear/" + k + nm]), "the resumed run is the straight run"
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "solver.npz")
    write(path, build_arrays())
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < 300 * 1024, "the fixture stays under 300 KB"
