"""The solver's contract restated for the tests (csrc/sgd.hip, m3d/solver.py; DESIGN "Solver"): the per-element update in NumPy, the
schedule, and derived single-step error bounds against an fp64 evaluation.

Update, fp32, every operation rounded once (fp32 arrays with np.float32 scalars: NumPy's ufuncs round each result once, no FMA):
    c = mscale m ;  w = wd p ;  d = (wd == 0) ? g : g + w ;  e = momentum c ;  m' = e + d ;  q = lr m' ;  p' = p - q
without a buffer (momentum == 0): p' = p - lr d.

Bounds.  u = 2^-24; fl(x) = x (1 + delta), |delta| <= u for a result in the normal range; a product below it (2^-126) may be rounded to
a subnormal or flushed: absolute error at most eta = 2^-126 instead.  Sums of fp32 values never lose to underflow.  Hats mark computed
values, plain letters the exact ones from the same (fp32) inputs and hyper-parameters.
    |c^ - c|  <= u |c| + eta
    |w^ - w|  <= u |w| + eta
    d^ = fl(g + w^):  |d^ - d| <= |w^ - w| + u |g + w^| <= (1 + u) |w^ - w| + u |d|          =: B      (wd == 0: d^ = d, B = 0)
    e^ = fl(mu c^):   |e^ - mu c| <= |mu| |c^ - c| + u |mu| |c^| + eta
                                  <= |mu| (u |c| + eta) (1 + u) + u |mu c| + eta               =: A
    m'^ = fl(e^ + d^): |m'^ - m'| <= A + B + u |e^ + d^| <= (1 + u) (A + B) + u |m'|           =: E_m
    q^ = fl(lr m'^):  |q^ - lr m'| <= |lr| E_m + u |lr m'^| + eta                              =: Q
    p'^ = fl(p - q^): |p'^ - p'|  <= Q + u |p - q^| <= (1 + u) Q + u |p'|                      =: E_p
To first order E_m = u (2 |mu c| + |w| + |d| + |m'|) and E_p = u (|lr m'^| + |p'|) + |lr| E_m.  Without a buffer m' = d, E_m = B.
The exact values are evaluated in fp64, whose own rounding (2^-53 per operation) is covered by the factor 1 + 2^-20 on each bound.
An implementation that contracts a product and a sum into one FMA drops one of the roundings above and stays within the same bounds."""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -20


def f32(x):
    return np.float32(x)


def step(p, g, m, lr, wd, momentum, mscale=1.0):
    """-> (p', m') of one update; p, g, m fp32 arrays (m None: no buffer, momentum must be 0), the rest scalars rounded to fp32 here"""
    lr, wd, mu, ms = f32(lr), f32(wd), f32(momentum), f32(mscale)
    assert p.dtype == np.float32 and g.dtype == np.float32 and (m is None or m.dtype == np.float32)
    with np.errstate(all="ignore"):
        d = g if wd == 0 else g + wd * p
        if m is None:
            assert mu == 0
            return p - lr * d, None
        c = ms * m
        m2 = mu * c + d
        return p - lr * m2, m2


def step64(p, g, m, lr, wd, momentum, mscale=1.0):
    """the same update in fp64 from the fp32 inputs and the fp32-rounded hyper-parameters"""
    lr, wd, mu, ms = (float(f32(v)) for v in (lr, wd, momentum, mscale))
    p, g = p.astype(np.float64), g.astype(np.float64)
    d = g if wd == 0 else g + wd * p
    if m is None:
        return p - lr * d, None
    m2 = mu * (ms * m.astype(np.float64)) + d
    return p - lr * m2, m2


def bounds(p, g, m, lr, wd, momentum, mscale, m_new32):
    """-> (E_p, E_m) of the module docstring, fp64 arrays; m_new32: the computed m' (d where there is no buffer) that q^ was formed from"""
    lr, wd, mu, ms = (float(f32(v)) for v in (lr, wd, momentum, mscale))
    p64, g64 = p.astype(np.float64), g.astype(np.float64)
    w = wd * p64
    d = g64 + w
    B = np.zeros_like(p64) if wd == 0 else (1 + U) * (U * np.abs(w) + ETA) + U * np.abs(d)
    if m is None:
        m_new, Em = d, B
    else:
        c = ms * m.astype(np.float64)
        A = abs(mu) * (U * np.abs(c) + ETA) * (1 + U) + U * np.abs(mu * c) + ETA
        m_new = mu * c + d
        Em = (1 + U) * (A + B) + U * np.abs(m_new)
    p_new = p64 - lr * m_new
    Q = abs(lr) * Em + U * np.abs(lr * m_new32.astype(np.float64)) + ETA
    Ep = (1 + U) * Q + U * np.abs(p_new)
    return Ep * SLACK, Em * SLACK


def check_step(p, g, m, lr, wd, momentum, mscale, p_new, m_new, what=""):
    """asserts that (p_new, m_new) - any fp32 implementation's result for these inputs - lies within the bounds of the fp64 evaluation;
    -> (largest |error| / bound of p', of m')"""
    p64, m64 = step64(p, g, m, lr, wd, momentum, mscale)
    if m is None:
        lr32, wd32 = f32(lr), f32(wd)
        with np.errstate(all="ignore"):
            m_used = g if wd32 == 0 else g + wd32 * p
    else:
        m_used = m_new
    Ep, Em = bounds(p, g, m, lr, wd, momentum, mscale, m_used)
    rp = np.abs(p_new.astype(np.float64) - p64) / Ep
    worst_p = float(rp.max()) if rp.size else 0.0
    assert worst_p <= 1.0, "%s: p' off by %.3g of its bound" % (what, worst_p)
    worst_m = 0.0
    if m is not None:
        rm = np.abs(m_new.astype(np.float64) - m64) / Em
        worst_m = float(rm.max()) if rm.size else 0.0
        assert worst_m <= 1.0, "%s: m' off by %.3g of its bound" % (what, worst_m)
    return worst_p, worst_m


def bits(a):
    """the bit patterns of an fp32 array, for bit-for-bit comparison"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------- schedule
class Schedule:
    """Warm-up, step decay and momentum correction restated from the SOLVER keys (a dict): begin(step) -> (lr of the non-bias group, lr
    of the bias group, correction factor handed to this step's update or 1.0).  Python doubles, in the order the solver applies them."""

    def __init__(self, keys, start_step=0, lr=0.0):
        self.c, self.lr, self.pending = dict(keys), lr, 1.0
        steps = self.c["STEPS"]
        self.k = len(steps)
        for i in range(1, len(steps)):
            if steps[i] >= start_step:
                self.k = i
                break

    def _update(self, new):
        c, lr = self.c, self.lr
        if new == lr:
            return
        ratio = max(new / max(lr, 1e-10), lr / max(new, 1e-10))
        if c["SCALE_MOMENTUM"] and lr > 1e-7 and ratio > c["SCALE_MOMENTUM_THRESHOLD"]:
            self.pending *= new / lr
        self.lr = new

    def begin(self, step):
        c = self.c
        W = c["WARM_UP_ITERS"]
        if step < W:
            alpha = step / W
            f = c["WARM_UP_FACTOR"] if c["WARM_UP_METHOD"] == "constant" else c["WARM_UP_FACTOR"] * (1 - alpha) + alpha
            self._update(c["BASE_LR"] * f)
        elif step == W:
            self._update(c["BASE_LR"])
        if self.k < len(c["STEPS"]) and step == c["STEPS"][self.k]:
            self._update(self.lr * c["GAMMA"])
            self.k += 1
        factor, self.pending = self.pending, 1.0
        return self.lr, (self.lr * 2 if c["BIAS_DOUBLE_LR"] else self.lr), factor


DEFAULT_KEYS = dict(BASE_LR=0.01, GAMMA=0.5, WEIGHT_DECAY=0.0001, STEPS=(0, 3000, 6000, 9000, 12000), MAX_ITER=12000, MOMENTUM=0.9,
                    BIAS_DOUBLE_LR=True, BIAS_WEIGHT_DECAY=False, WEIGHT_DECAY_GN=0.0, WARM_UP_ITERS=500, WARM_UP_FACTOR=1.0 / 3.0,
                    WARM_UP_METHOD="linear", SCALE_MOMENTUM=True, SCALE_MOMENTUM_THRESHOLD=1.1)
SHORT = dict(WARM_UP_ITERS=5, STEPS=(0, 8, 14, 20), MAX_ITER=20)
# case -> (dataset, overrides of its SOLVER keys, step after which the run is saved and resumed or None, full trajectory recorded)
CASES = {
    "nuclei_full": ("nuclei", {}, None, False),
    "soma_full": ("soma", dict(STEPS=(0, 3000, 6000, 9000), MAX_ITER=9000), None, False),
    "short_linear": ("nuclei", dict(SHORT), None, True),
    "short_constant": ("nuclei", dict(SHORT, WARM_UP_METHOD="constant"), None, True),
    "short_nowarm": ("nuclei", dict(SHORT, WARM_UP_ITERS=0), None, True),
    "short_resume": ("nuclei", dict(SHORT), 10, True),
}
SHORT_CASES = [k for k, v in CASES.items() if v[3]]
# the tiny model of the fixture: name -> shape, in named_parameters order; 40 values
MODEL = (("fc1.weight", (4, 5)), ("fc1.bias", (5,)), ("fc2.weight", (5, 2)), ("fc2.bias", (5,)))


def keys_of(case):
    k = dict(DEFAULT_KEYS)
    k.update(CASES[case][1])
    return k


def load_case(npz, case):
    """the arrays of one case of tests/golden/solver.npz (tests/golden/gen_solver.py) as a dict without the case prefix"""
    pre = case + "/"
    return {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}


def solver_cfg(case, **more):
    """the m3d.SolverCfg of a case"""
    import m3d
    kw = dict(CASES[case][1])
    kw.update(more)
    return (m3d.SolverCfg.soma if CASES[case][0] == "soma" else m3d.SolverCfg.nuclei)(**kw)
