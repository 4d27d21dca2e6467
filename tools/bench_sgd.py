#!/usr/bin/env python3
"""Times one solver step on the parameter set of the nuclei detector (the tensors of m3d.synth.make_params: width 32, hidden 1024) -
96.3 M parameters, 89.9 M of them Box_Head.fc1.weight - with synthetic gradients: m3d.Solver.step() (one fused launch, csrc/sgd.hip or
csrc/adam.hip) beside torch.optim.SGD / torch.optim.Adam (`--optimizer`) on the same groups, foreach=True and, where this torch offers
it, fused=True.

Situations: a plain step; under SGD a step right after a learning-rate decay, where the momentum buffers are scaled first; with
`--clip NORM` a step behind the global-norm gradient clip.  After a decay m3d.Solver hands the factor to the same launch; beside
torch.optim.SGD the buffers are multiplied one by one, as the reference's _CorrectMomentum does (lib/utils/net.py:86-99).  The factor
alternates between 0.5 and 2 so that the values stay where they are.  Clipped, m3d.Solver(CLIP_NORM=NORM) runs its coefficient pass and
hands the device scalar to the update; beside torch it is torch.nn.utils.clip_grad_norm_ and then the step.  NORM is a fraction of the
gradients' norm (default 0.5), so the clip is active; torch scales its gradients in place, so there it is active on the first step only
and multiplies by 1 afterwards - the same work.

Per situation: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each measurement is the time
between two device events around `--inner` consecutive steps, divided by `--inner`; median and spread (min .. max) in ms.  That is the
time of a step as a user sees it on an idle stream: device work where the kernels take longer than the host needs to issue them, host
issue time (Python, ctypes, the optimiser's own bookkeeping) where they do not.
"MB" is what each variant must move, counted from the sizes (N = 4 bytes x elements, Nd = the part that decays):
  SGD   m3d          5 N: read p, g, m, write p, m - with or without the buffer scale
        torch fused  5 N, and after a decay 2 N more for the separate multiplication of the buffers
        torch foreach  3 Nd (g += wd p) + 2 N (buf *= momentum) + 3 N (buf += g) + 3 N (p -= lr buf), and 2 N more after a decay
  Adam  m3d, torch fused  7 N: read p, g, m, v, write p, m, v
        torch foreach  3 Nd (g + wd p) + 3 N (lerp) + 2 N (v *= beta2) + 3 N (addcmul) + 2 N (sqrt) + 2 N (/ bc2) + 2 N (+ eps) + 4 N (addcdiv)
  clipped: m3d 1 N more (the coefficient pass reads g); torch 3 N more (the norms read g, the scaling reads and writes it)
and the fraction of 6.3 TB/s = those bytes over the median over the HBM peak: an accounting figure, not a counter reading.
Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
HBM_PEAK = 6.3e12
PLAIN, DECAY, CLIPPED = "plain", "after a decay", "clipped"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="steps per timed window")
    ap.add_argument("--optimizer", choices=("SGD", "Adam"), default="SGD")
    ap.add_argument("--clip", type=float, nargs="?", const=0.5, default=None,
                    help="also time a clipped step; the clip norm as a fraction of the gradients' norm (default 0.5)")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import m3d
    assert torch.cuda.is_available(), "bench_sgd needs a GPU"
    adam = a.optimizer == "Adam"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    torch.manual_seed(0)
    cfg = m3d.SolverCfg(TYPE=a.optimizer)
    rate = cfg.BASE_LR

    def parameter_set():
        from m3d.synth import make_params
        det = [(k, torch.nn.Parameter(v.cuda())) for k, v in make_params(mlp_dim=a.hidden).items() if "running_" not in k]
        for _, p in det:
            p.grad = torch.randn_like(p) * 0.01
        return det

    variants = {}                                   # name -> (step(situation, factor), bytes moved(situation))
    det = parameter_set()
    solver = m3d.Solver(det, cfg)
    solver.begin_step(cfg.WARM_UP_ITERS)              # BASE_LR on both groups' terms
    solver.mscale = 1.0
    elements = sum(p.numel() for g in solver.param_groups for p in g["params"])
    decayed = sum(p.numel() for g in solver.param_groups if g["weight_decay"] != 0 for p in g["params"])
    N, Nd = 4.0 * elements, 4.0 * decayed
    clip_norm = None
    clipped = None
    if a.clip is not None:
        clip_norm = a.clip * float(torch.sqrt(sum((p.grad.double() ** 2).sum() for _, p in det)))
        det_c = parameter_set()
        clipped = m3d.Solver(det_c, m3d.SolverCfg(TYPE=a.optimizer, CLIP_NORM=clip_norm))
        clipped.begin_step(cfg.WARM_UP_ITERS)
        clipped.mscale = 1.0
    passes = 7 if adam else 5

    def m3d_step(situation, factor):
        s = clipped if situation == CLIPPED else solver
        if factor is not None:
            s.mscale = factor
        s.step()
    variants["m3d.Solver"] = (m3d_step, lambda situation: passes * N + (N if situation == CLIPPED else 0))
    for name, kw in (("torch foreach", dict(foreach=True)), ("torch fused", dict(fused=True))):
        d = parameter_set()
        named = dict(d)
        groups = [dict(params=[q for n, q in named.items() if "bias" not in n], lr=rate, weight_decay=cfg.WEIGHT_DECAY),
                  dict(params=[q for n, q in named.items() if "bias" in n], lr=2 * rate, weight_decay=0)]
        try:
            if adam:
                opt = torch.optim.Adam(groups, betas=cfg.BETAS, eps=cfg.EPS, **kw)
            else:
                opt = torch.optim.SGD(groups, momentum=cfg.MOMENTUM, **kw)
            opt.step()
        except (RuntimeError, TypeError, ValueError) as e:
            say("# %s: not offered by this torch (%s)" % (name, str(e).splitlines()[0][:100]))
            continue

        def torch_step(situation, factor, opt=opt, d=d):
            if factor is not None:
                for _, q in d:
                    opt.state[q]["momentum_buffer"] *= factor
            if situation == CLIPPED:
                torch.nn.utils.clip_grad_norm_([q for _, q in d], clip_norm)
            opt.step()
        if "fused" in name:
            base = passes * N
        else:
            base = 3 * Nd + (18 * N if adam else 8 * N)

        def moved(situation, base=base):
            return base + (2 * N if situation == DECAY else 0) + (3 * N if situation == CLIPPED else 0)
        variants[name] = (torch_step, moved)

    say("# one %s step, Detector(nuclei, width %d, hidden %d): %d tensors, %d elements (%.1f MB), %d of them decay"
        % (a.optimizer, 32, a.hidden, sum(len(g["params"]) for g in solver.param_groups), elements, N / 1e6, decayed))
    say("# %d warm-up + %d alternating repetitions of %d steps; time per step between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# MB = bytes the variant must move (from the sizes); HBM = MB / median / 6.3 TB/s")
    if clip_norm is not None:
        say("# clipped: clip norm %.6g = %.3g of the gradients' norm" % (clip_norm, a.clip))
    say("%-14s %-16s | %-28s %8s %6s" % ("situation", "variant", "ms per step", "MB", "HBM"))

    def timed(fn, situation, i):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for k in range(a.inner):
            fn(situation, (0.5 if (i * a.inner + k) % 2 == 0 else 2.0) if situation == DECAY else None)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner
    situations = [PLAIN] + ([] if adam else [DECAY]) + ([CLIPPED] if clip_norm is not None else [])
    results = {}
    for situation in situations:
        times = {name: [] for name in variants}
        names = list(variants)
        for i in range(a.warmup + a.reps):
            order = names[i % len(names):] + names[:i % len(names)]
            for name in order:
                t = timed(variants[name][0], situation, i)
                if i >= a.warmup:
                    times[name].append(t)
        for name in names:
            med, mb = statistics.median(times[name]), variants[name][1](situation) / 1e6
            results[(situation, name)] = (med, min(times[name]), max(times[name]))
            say("%-14s %-16s | %-28s %8.1f %5.1f%%" % (situation, name, "%.3f (%.3f .. %.3f)" % (med, min(times[name]), max(times[name])), mb,
                                                       100.0 * mb * 1e6 / (med * 1e-3) / HBM_PEAK))
    for situation in situations:
        mine = results[(situation, "m3d.Solver")]
        others = {n: r for (si, n), r in results.items() if si == situation and n != "m3d.Solver"}
        if others:
            best = min(others, key=lambda n: others[n][0])
            theirs = others[best]
            apart = abs(mine[0] - theirs[0]) > (mine[2] - mine[1]) + (theirs[2] - theirs[1])
            say("# %s: m3d.Solver / best torch variant (%s) = %.2f; spreads %.3f .. %.3f against %.3f .. %.3f ms: %s"
                % (situation, best, mine[0] / theirs[0], mine[1], mine[2], theirs[1], theirs[2],
                   "apart by more than the sum of the spreads" if apart else "NOT apart by more than the sum of the spreads"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
