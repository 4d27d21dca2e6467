#!/usr/bin/env python3
"""Times one solver step on the parameter set of the nuclei detector (the tensors of m3d.synth.make_params: width 32, hidden 1024) -
96.3 M parameters, 89.9 M of them Box_Head.fc1.weight - with synthetic gradients: m3d.Solver.step() (one fused launch, csrc/sgd.hip)
beside torch.optim.SGD on the same groups, foreach=True and, where this torch offers it, fused=True.

Two situations: a plain step, and a step right after a learning-rate decay, where the momentum buffers are scaled first.  m3d.Solver
hands the factor to the same launch; beside torch.optim.SGD the buffers are multiplied one by one, as the reference's _CorrectMomentum
does (lib/utils/net.py:86-99).  The factor alternates between 0.5 and 2 so that the values stay where they are.

Per situation: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each measurement is the time
between two device events around `--inner` consecutive steps, divided by `--inner`; median and spread (min .. max) in ms.  That is the
time of a step as a user sees it on an idle stream: device work where the kernels take longer than the host needs to issue them, host
issue time (Python, ctypes, the optimiser's own bookkeeping) where they do not.
"MB" is what each variant must move, counted from the sizes (N = 4 bytes x elements, Nd = the part that decays):
  m3d          5 N: read p, g, m, write p, m - with or without the buffer scale
  torch fused  5 N, and after a decay 2 N more for the separate multiplication of the buffers
  torch foreach  3 Nd (g += wd p) + 2 N (buf *= momentum) + 3 N (buf += g) + 3 N (p -= lr buf), and 2 N more after a decay
and the fraction of 6.3 TB/s = those bytes over the median over the HBM peak: an accounting figure, not a counter reading.
Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
HBM_PEAK = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="steps per timed window")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import m3d
    assert torch.cuda.is_available(), "bench_sgd needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    torch.manual_seed(0)
    cfg = m3d.SolverCfg.nuclei()
    rate = cfg.BASE_LR

    def parameter_set():
        from m3d.synth import make_params
        det = [(k, torch.nn.Parameter(v.cuda())) for k, v in make_params(mlp_dim=a.hidden).items() if "running_" not in k]
        for _, p in det:
            p.grad = torch.randn_like(p) * 0.01
        return det

    variants = {}
    det = parameter_set()
    solver = m3d.Solver(det, cfg)
    solver.begin_step(cfg.WARM_UP_ITERS)              # BASE_LR on both groups' terms
    solver.mscale = 1.0
    elements = sum(p.numel() for g in solver.param_groups for p in g["params"])
    decayed = sum(p.numel() for g in solver.param_groups if g["weight_decay"] != 0 for p in g["params"])
    N, Nd = 4.0 * elements, 4.0 * decayed

    def m3d_step(factor):
        if factor is not None:
            solver.mscale = factor
        solver.step()
    variants["m3d.Solver"] = (m3d_step, det, lambda after: 5 * N)
    for name, kw in (("torch foreach", dict(foreach=True)), ("torch fused", dict(fused=True))):
        d = parameter_set()
        named = dict(d)
        groups = [dict(params=[q for n, q in named.items() if "bias" not in n], lr=rate, weight_decay=cfg.WEIGHT_DECAY),
                  dict(params=[q for n, q in named.items() if "bias" in n], lr=2 * rate, weight_decay=0)]
        try:
            opt = torch.optim.SGD(groups, momentum=cfg.MOMENTUM, **kw)
            opt.step()
        except (RuntimeError, TypeError, ValueError) as e:
            say("# %s: not offered by this torch (%s)" % (name, str(e).splitlines()[0][:100]))
            continue

        def torch_step(factor, opt=opt, d=d):
            if factor is not None:
                for _, q in d:
                    opt.state[q]["momentum_buffer"] *= factor
            opt.step()
        moved = (lambda after: 5 * N + (2 * N if after else 0)) if "fused" in name else (lambda after: 3 * Nd + 8 * N + (2 * N if after else 0))
        variants[name] = (torch_step, d, moved)

    say("# one solver step, Detector(nuclei, width %d, hidden %d): %d tensors, %d elements (%.1f MB), %d of them decay"
        % (32, a.hidden, sum(len(g["params"]) for g in solver.param_groups), elements, N / 1e6, decayed))
    say("# %d warm-up + %d alternating repetitions of %d steps; time per step between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# MB = bytes the variant must move (from the sizes); HBM = MB / median / 6.3 TB/s")
    say("%-14s %-16s | %-28s %8s %6s" % ("situation", "variant", "ms per step", "MB", "HBM"))

    def timed(fn, after, i):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(a.inner):
            fn((0.5 if (i * a.inner + k) % 2 == 0 else 2.0) if after else None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner
    results = {}
    for after in (False, True):
        times = {name: [] for name in variants}
        names = list(variants)
        for i in range(a.warmup + a.reps):
            order = names[i % len(names):] + names[:i % len(names)]
            for name in order:
                t = timed(variants[name][0], after, i)
                if i >= a.warmup:
                    times[name].append(t)
        for name in names:
            med, mb = statistics.median(times[name]), variants[name][2](after) / 1e6
            results[(after, name)] = (med, min(times[name]), max(times[name]))
            say("%-14s %-16s | %-28s %8.1f %5.1f%%" % ("after a decay" if after else "plain", name,
                                                       "%.3f (%.3f .. %.3f)" % (med, min(times[name]), max(times[name])), mb,
                                                       100.0 * mb * 1e6 / (med * 1e-3) / HBM_PEAK))
    for after in (False, True):
        mine = results[(after, "m3d.Solver")]
        others = {n: r for (af, n), r in results.items() if af == after and n != "m3d.Solver"}
        if others:
            best = min(others, key=lambda n: others[n][0])
            say("# %s: m3d.Solver / best torch variant (%s) = %.2f; spreads %.3f .. %.3f against %.3f .. %.3f ms"
                % ("after a decay" if after else "plain", best, mine[0] / others[best][0], mine[1], mine[2], others[best][1], others[best][2]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
