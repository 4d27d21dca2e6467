"""The reference's solver: SGD or Adam with its parameter groups, warm-up, step decay and (SGD) momentum correction, on one fused update
launch (csrc/sgd.hip, csrc/adam.hip), an optional global-norm gradient clip that stays on the device, and its checkpoints.

Reference: tools/train_net_step.py:286-489 (groups, the optimiser choice at :330-333, schedule, loop order, save_ckpt at :122-139) and
lib/utils/net.py:35-107 (clip_gradient, update_learning_rate, _CorrectMomentum).  DESIGN ("Solver") has the contract.  Construction, the
schedule and the state dicts are host logic and work on CPU parameters; only step() needs the device."""
import math
import os

import torch

from . import ops

__all__ = ["SolverCfg", "Solver", "save_ckpt", "load_ckpt"]


class SolverCfg:
    """The SOLVER keys (and TRAIN.SNAPSHOT_ITERS) the solver reads; defaults = the nuclei YAML merged over lib/core/config.py."""

    def __init__(self, **kw):
        self.TYPE = "SGD"                                   # or "Adam" (train_net_step.py:330-333)
        self.LR_POLICY = "steps_with_decay"
        self.BASE_LR = 0.01
        self.GAMMA = 0.5
        self.WEIGHT_DECAY = 0.0001
        self.STEPS = (0, 3000, 6000, 9000, 12000)
        self.MAX_ITER = 12000
        self.MOMENTUM = 0.9                                 # config.py:588
        self.BIAS_DOUBLE_LR = True                          # config.py:596
        self.BIAS_WEIGHT_DECAY = False                      # config.py:599
        self.WEIGHT_DECAY_GN = 0.0                          # config.py:593
        self.WARM_UP_ITERS = 500                            # config.py:602
        self.WARM_UP_FACTOR = 1.0 / 3.0                     # config.py:605
        self.WARM_UP_METHOD = "linear"                      # config.py:608
        self.SCALE_MOMENTUM = True                          # config.py:612
        self.SCALE_MOMENTUM_THRESHOLD = 1.1                 # config.py:616
        self.SNAPSHOT_ITERS = 3000                          # TRAIN.SNAPSHOT_ITERS
        self.BETAS = (0.9, 0.999)                           # Adam: torch.optim.Adam's defaults, which the reference leaves alone
        self.EPS = 1e-8
        self.CLIP_NORM = None                               # the clip_norm of clip_gradient (lib/utils/net.py:35-47); None: no clip
        unknown = sorted(set(kw) - set(self.__dict__))
        if unknown:
            raise TypeError("SolverCfg: unknown key(s) %s (known: %s)" % (", ".join(unknown), ", ".join(sorted(self.__dict__))))
        self.__dict__.update(kw)
        self.STEPS = tuple(int(s) for s in self.STEPS)
        self.BETAS = tuple(float(b) for b in self.BETAS)
        if self.TYPE not in ("SGD", "Adam"):
            raise ValueError("SolverCfg: SOLVER.TYPE %r is not built (SGD and Adam only)" % (self.TYPE,))
        if self.LR_POLICY != "steps_with_decay":
            raise ValueError("SolverCfg: SOLVER.LR_POLICY %r is not built (steps_with_decay only)" % (self.LR_POLICY,))
        if len(self.BETAS) != 2 or not all(0.0 <= b < 1.0 for b in self.BETAS) or not self.EPS > 0:
            raise ValueError("SolverCfg: BETAS must be two values in [0, 1) and EPS positive")
        if self.CLIP_NORM is not None and not (self.CLIP_NORM > 0 and math.isfinite(self.CLIP_NORM)):
            raise ValueError("SolverCfg: CLIP_NORM must be None or positive and finite")

    # what the soma YAML changes: SolverCfg(TYPE="Adam", **SolverCfg.SOMA) is its schedule under Adam
    SOMA = dict(STEPS=(0, 3000, 6000, 9000), MAX_ITER=9000)

    @staticmethod
    def _shipped(name, kw):
        """nuclei() and soma() are the two shipped YAML files, both SGD runs, and keep refusing another TYPE as they always have; a
        configuration of another type is built with SolverCfg(TYPE=..., ...) itself"""
        if kw.get("TYPE", "SGD") != "SGD":
            raise ValueError("SolverCfg.%s: the shipped configuration is an SGD run; build SOLVER.TYPE %r with SolverCfg(TYPE=..., ...)"
                             % (name, kw["TYPE"]))
        return SolverCfg(**kw)

    @staticmethod
    def nuclei(**kw):
        return SolverCfg._shipped("nuclei", kw)

    @staticmethod
    def soma(**kw):
        d = dict(SolverCfg.SOMA)
        d.update(kw)
        return SolverCfg._shipped("soma", d)


def _group_defaults(kind="SGD"):
    """the hyper-parameter keys of a torch.optim.SGD / torch.optim.Adam group of this torch, with their defaults"""
    d = dict(getattr(torch.optim, kind)([torch.zeros(1)], lr=0.0).state_dict()["param_groups"][0])
    d.pop("params")
    return d


_ADAM_REFUSED = ("amsgrad", "maximize", "decoupled_weight_decay")


class Solver:
    """torch.optim.SGD, or with cfg.TYPE == "Adam" torch.optim.Adam, as the reference builds and drives it.

    named_parameters: (name, parameter) pairs, e.g. model.named_parameters().  requires_grad parameters with `bias` in the name form the
    bias group (twice the rate if BIAS_DOUBLE_LR, no decay unless BIAS_WEIGHT_DECAY), the rest the non-bias group; the GroupNorm group is
    kept and empty.  Loop order: begin_step(step), zero_grad(), forward, backward, step().  stats=True also fills `grad_sq` (sum of g^2
    over the gradients of the step, fp64) and `nonfinite` (their non-finite elements) on the device.  With cfg.CLIP_NORM the gradients
    enter the update scaled by `clip_coef` = CLIP_NORM / max(sqrt(grad_sq), CLIP_NORM), a device scalar that a pass over the gradients
    writes in front of the update; nothing is read back, and the two statistics are there whatever `stats` says."""

    def __init__(self, named_parameters, cfg, start_step=0, stats=False):
        self.cfg = cfg
        self.adam = cfg.TYPE == "Adam"
        nonbias, bias = [], []
        for name, p in named_parameters:
            if p.requires_grad:
                (bias if "bias" in name else nonbias).append(p)
        params = nonbias + bias
        if not params:
            raise ValueError("Solver: no parameter requires a gradient")
        dev = params[0].device
        if any(p.device != dev or p.dtype != torch.float32 for p in params):
            raise ValueError("Solver: the parameters must be fp32 on one device")
        hyper = _group_defaults(cfg.TYPE)
        if self.adam:
            hyper.update(betas=cfg.BETAS, eps=cfg.EPS)
            assert not any(hyper.get(k) for k in _ADAM_REFUSED)
        else:
            hyper.update(momentum=cfg.MOMENTUM, dampening=0, nesterov=False)

        def group(ps, lr, wd):
            g = dict(hyper)
            g.update(params=ps, lr=lr, weight_decay=wd)
            return g
        self.param_groups = [group(nonbias, 0, cfg.WEIGHT_DECAY),
                             group(bias, 0 * (cfg.BIAS_DOUBLE_LR + 1), cfg.WEIGHT_DECAY if cfg.BIAS_WEIGHT_DECAY else 0),
                             group([], 0, cfg.WEIGHT_DECAY_GN)]
        self._params = params
        # one flat buffer; every view starts on a 16-byte boundary, so the update kernel reads and writes it in quads
        offs, at = [], 0
        for p in params:
            offs.append(at)
            at += (p.numel() + 3) // 4 * 4

        def flat():
            f = torch.zeros((at,), dtype=torch.float32, device=dev)
            return f, [f[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]
        self._flat, self._bufs = flat()          # SGD: the momentum buffers; Adam: exp_avg
        if self.adam:
            self._flat2, self._bufs2 = flat()    # exp_avg_sq
        self._live = [False] * len(params)       # torch creates a parameter's buffer at its first step with a gradient
        self._steps = [0] * len(params)          # Adam: torch's state['step'], the steps at which the parameter had a gradient
        clip = cfg.CLIP_NORM is not None
        self._stats = torch.zeros((2,), dtype=torch.float64, device=dev) if (stats or clip) else None
        self._coef = torch.ones((1,), dtype=torch.float32, device=dev) if clip else None
        self.lr = self.param_groups[0]["lr"]
        self.mscale = 1.0                        # pending momentum correction: handed to the next launch, then 1 again (SGD only)
        self.start_step = start_step

    # ------------------------------------------------------------------ schedule
    @property
    def start_step(self):
        return self._start_step

    @start_step.setter
    def start_step(self, step):
        steps = self.cfg.STEPS
        self._start_step = int(step)
        self.k = len(steps)
        for i in range(1, len(steps)):
            if steps[i] >= step:
                self.k = i
                break

    def _update(self, new):
        lr, c = self.lr, self.cfg
        if new == lr:
            return
        ratio = max(new / max(lr, 1e-10), lr / max(new, 1e-10))
        for i, g in enumerate(self.param_groups):
            g["lr"] = new * 2 if (i == 1 and c.BIAS_DOUBLE_LR) else new
        if not self.adam and c.SCALE_MOMENTUM and lr > 1e-7 and ratio > c.SCALE_MOMENTUM_THRESHOLD:      # net.py:81: SGD only
            self.mscale *= new / lr
        self.lr = new

    def begin_step(self, step):
        """The rate of `step`: warm-up, then the decay steps, each with its momentum correction (train_net_step.py:409-436)."""
        c = self.cfg
        if step < c.WARM_UP_ITERS:
            if c.WARM_UP_METHOD == "constant":
                f = c.WARM_UP_FACTOR
            elif c.WARM_UP_METHOD == "linear":
                alpha = step / c.WARM_UP_ITERS
                f = c.WARM_UP_FACTOR * (1 - alpha) + alpha
            else:
                raise KeyError("Unknown SOLVER.WARM_UP_METHOD: {}".format(c.WARM_UP_METHOD))
            self._update(c.BASE_LR * f)
        elif step == c.WARM_UP_ITERS:
            self._update(c.BASE_LR)
        if self.k < len(c.STEPS) and step == c.STEPS[self.k]:
            self._update(self.lr * c.GAMMA)
            self.k += 1
        return self.lr

    # ------------------------------------------------------------------ the update
    @property
    def grad_sq(self):
        return None if self._stats is None else self._stats[0]

    @property
    def nonfinite(self):
        return None if self._stats is None else self._stats[1]

    @property
    def clip_coef(self):
        """the coefficient the last step() scaled its gradients by: a 0-d device tensor, None without CLIP_NORM"""
        return None if self._coef is None else self._coef[0]

    def zero_grad(self):
        for p in self._params:
            p.grad = None

    def step(self):
        """With CLIP_NORM one ops.grad_clip_coef pass, then one ops.sgd_step / ops.adam_step launch, on the current stream over every
        parameter that has a gradient; then the cached conv / linear packs are dropped: the kernels write through raw pointers and do
        not bump `_version`."""
        ps, gs, ms, vs, lrs, wds, steps, stepped = [], [], [], [], [], [], [], []
        momentum = 0 if self.adam else self.param_groups[0]["momentum"]
        i = 0
        for g in self.param_groups:
            for p in g["params"]:
                if p.grad is not None:
                    if not p.is_cuda:
                        raise ops.M3DError("Solver.step: needs CUDA (ROCm) parameters; there is no CPU path")
                    ps.append(p.detach())
                    gs.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
                    ms.append(self._bufs[i])
                    lrs.append(g["lr"])
                    wds.append(g["weight_decay"])
                    stepped.append(i)
                    if self.adam:
                        vs.append(self._bufs2[i])
                        steps.append(self._steps[i] + 1)
                    else:
                        self._live[i] = momentum != 0            # torch keeps no buffer without momentum
                elif not self.adam and self._live[i] and self.mscale != 1.0:
                    self._bufs[i].mul_(self.mscale)          # the correction reaches a buffer whose parameter sits this step out
                i += 1
        clip = self._coef is not None
        if clip:
            ops.grad_clip_coef(gs, self.cfg.CLIP_NORM, self._stats, self._coef)
        if self.adam:
            g0 = self.param_groups[0]
            ops.adam_step(ps, gs, ms, vs, lrs, wds, steps, g0["betas"], g0["eps"], None if clip else self._stats, self._coef)
            for i in stepped:
                self._steps[i] += 1
                self._live[i] = True
        elif clip:
            ops.sgd_step_scaled(ps, gs, ms if momentum != 0 else None, lrs, wds, momentum, self.mscale, None, self._coef)
        else:
            ops.sgd_step(ps, gs, ms if momentum != 0 else None, lrs, wds, momentum, self.mscale, self._stats)
        self.mscale = 1.0
        from . import compat
        compat.invalidate_packs()

    # ------------------------------------------------------------------ torch.optim.SGD's / torch.optim.Adam's state dict
    def state_dict(self):
        state, groups, at = {}, [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != "params"}
            d["params"] = list(range(at, at + len(g["params"])))
            at += len(g["params"])
            groups.append(d)
        for i, b in enumerate(self._bufs):
            if not self._live[i]:
                continue
            if self.adam:
                state[i] = {"step": torch.tensor(float(self._steps[i]), dtype=torch.float32), "exp_avg": b.clone(),
                            "exp_avg_sq": self._bufs2[i].clone()}
            else:
                state[i] = {"momentum_buffer": b * self.mscale if self.mscale != 1.0 else b.clone()}
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != len(self.param_groups) or any(len(a["params"]) != len(b["params"]) for a, b in zip(groups, self.param_groups)):
            raise ValueError("Solver.load_state_dict: the saved parameter groups do not match this model's")
        if any(("betas" in g) != self.adam for g in groups):
            raise ValueError("Solver.load_state_dict: the saved state is %s's, this solver is %s"
                             % (("torch.optim.SGD", "Adam") if self.adam else ("torch.optim.Adam", "SGD")))
        if self.adam:
            if any(g.get(k) for g in groups for k in _ADAM_REFUSED):
                raise ValueError("Solver.load_state_dict: %s are not built" % ", ".join(_ADAM_REFUSED))
            if len({(tuple(float(b) for b in g["betas"]), float(g["eps"])) for g in groups}) != 1:
                raise ValueError("Solver.load_state_dict: one betas and eps for all groups")
        elif len({float(g.get("momentum", 0)) for g in groups}) != 1:
            raise ValueError("Solver.load_state_dict: one momentum for all groups")
        for mine, saved in zip(self.param_groups, groups):
            mine.update({k: v for k, v in saved.items() if k != "params"})
            if self.adam:
                mine["betas"] = tuple(float(b) for b in mine["betas"])
        order = [j for g in groups for j in g["params"]]       # saved index of our parameter i
        with torch.no_grad():
            for i, j in enumerate(order):
                st = sd["state"].get(j)
                if self.adam:
                    if st is not None and st.get("exp_avg") is not None:
                        self._bufs[i].copy_(st["exp_avg"].reshape(self._bufs[i].shape))
                        self._bufs2[i].copy_(st["exp_avg_sq"].reshape(self._bufs[i].shape))
                        self._steps[i] = int(round(float(st["step"])))
                        self._live[i] = True
                    else:
                        self._bufs[i].zero_()
                        self._bufs2[i].zero_()
                        self._steps[i] = 0
                        self._live[i] = False
                elif st is not None and st.get("momentum_buffer") is not None:
                    self._bufs[i].copy_(st["momentum_buffer"].reshape(self._bufs[i].shape))
                    self._live[i] = True
                else:
                    self._bufs[i].zero_()
                    self._live[i] = False
        self.lr = self.param_groups[0]["lr"]
        self.mscale = 1.0


def save_ckpt(output_dir, step, model, solver, train_size=0, batch_size=1):
    """The reference's checkpoint (train_net_step.py:122-139): output_dir/ckpt/model_step{step}.pth.  -> its path"""
    ckpt_dir = os.path.join(output_dir, "ckpt")
    os.makedirs(ckpt_dir, exist_ok=True)
    path = os.path.join(ckpt_dir, "model_step{}.pth".format(step))
    torch.save({"step": step, "train_size": train_size, "batch_size": batch_size, "model": model.state_dict(),
                "optimizer": solver.state_dict()}, path)
    return path


def load_ckpt(path, model, solver=None):
    """Loads the model, and the solver if one is given, from a checkpoint of save_ckpt or of the reference.  -> the step to resume at,
    `step + 1` (train_net_step.py:343); the solver's decay index is set for it."""
    ckpt = torch.load(path, map_location="cpu")
    model.load_state_dict(ckpt["model"])
    start = int(ckpt["step"]) + 1
    if solver is not None:
        solver.load_state_dict(ckpt["optimizer"])
        solver.start_step = start
    return start
