"""The Adam update and the gradient clip restated for the tests (csrc/adam.hip, m3d/solver.py; DESIGN "Solver"): the per-element update
in NumPy, its fp64 evaluation, derived single-step error bounds, the statistics tree and the clip coefficient.

Update, fp32, every operation rounded once (fp32 arrays with np.float32 scalars: NumPy's ufuncs round each result once, no FMA; its
fp32 square root and division are correctly rounded).  Host scalars, in Python doubles as torch.optim.Adam forms them, then rounded to
fp32:  lr_step = lr / (1 - b1^t),  bc2 = (1 - b2^t)^0.5,  o1 = 1 - b1,  o2 = 1 - b2,  b2,  eps.  s is the clip coefficient (fp32).
    a = s g  (only with s) ;  w = wd p ;  d = (wd == 0) ? a : a + w ;  e = d - m ;  f = o1 e ;  m' = m + f ;
    r = d d ;  x = b2 v ;  y = o2 r ;  v' = x + y ;  z = sqrt(v') ;  t = z / bc2 ;  q = t + eps ;  k = m' / q ;  h = lr_step k ;  p' = p - h

Bounds.  u = 2^-24; fl(x) = x (1 + delta), |delta| <= u for a result in the normal range.  A product or quotient whose exact value lies
below it may be rounded to a subnormal or flushed: absolute error at most eta = 2^-126 instead, written und(.) below and counted only
where the value, with the error it inherits, can lie under 2^-125 and is not an exact zero.  Sums, differences and square roots of fp32
values never lose to underflow.  Hats mark computed values, plain letters the exact ones from the same fp32 inputs and scalars.
    E_a = u |a| + und                                                           (no s: a = g, E_a = 0)
    E_w = u |w| + und
    d^ = fl(a^ + w^):   |d^ - d| <= E_a + E_w + u |a^ + w^| <= (1 + u)(E_a + E_w) + u |d|             =: E_d    (wd == 0: E_d = E_a)
    e^ = fl(d^ - m):    |e^ - e| <= E_d + u |d^ - m|        <= (1 + u) E_d + u |e|                    =: E_e
    f^ = fl(o1 e^):     |f^ - f| <= o1 E_e + u |o1 e^| + und <= (1 + u) o1 E_e + u |f| + und          =: E_f
    m'^ = fl(m + f^):   |m'^ - m'| <= E_f + u |m + f^|      <= (1 + u) E_f + u |m'|                   =: E_m
    r^ = fl(d^ d^):     |d^2 - d^ d^| <= E_d (2 |d| + E_d) =: G;  |r^ - r| <= (1 + u) G + u |r| + und =: E_r
    x^ = fl(b2 v):      |x^ - x| <= u |x| + und                                                       =: E_x
    y^ = fl(o2 r^):     |y^ - y| <= (1 + u) o2 E_r + u |y| + und                                      =: E_y
    v'^ = fl(x^ + y^):  |v'^ - v'| <= (1 + u)(E_x + E_y) + u |v'|                                     =: E_v
    z^ = fl(sqrt(v'^)): |sqrt(v'^) - sqrt(v')| = |v'^ - v'| / (sqrt(v'^) + sqrt(v')) <= min(E_v / sqrt(v'), sqrt(E_v)) =: S
                        |z^ - z| <= (1 + u) S + u z                                                   =: E_z
    t^ = fl(z^ / bc2):  |t^ - t| <= (1 + u) E_z / bc2 + u t + und                                     =: E_t
    q^ = fl(t^ + eps):  |q^ - q| <= (1 + u) E_t + u q                                                 =: E_q
    k^ = fl(m'^ / q^):  m'^/q^ - m'/q = (m'^ - m')/q^ + m' (q - q^)/(q q^), q^ >= q - E_q > 0:
                        |m'^/q^ - k| <= (E_m + |k| E_q) / (q - E_q) =: D;  |k^ - k| <= (1 + u) D + u |k| + und     =: E_k
    h^ = fl(lr_step k^): |h^ - h| <= (1 + u) |lr_step| E_k + u |h| + und                              =: E_h
    p'^ = fl(p - h^):   |p'^ - p'| <= E_h + u |p - h^| <= (1 + u) E_h + u |p'|                        =: E_p
To first order, without s or decay: E_m = u (o1 |e| + |f| + |m'|), E_v = u (|x| + 2 |y| + |v'|), E_p = u (2 |h| + |p'|) + |lr_step| (E_m +
|k| E_q) / q.  The exact values are evaluated in fp64, whose own rounding (2^-53 per operation) is covered by the factor 1 + 2^-20 on each
bound.  An implementation that contracts a product and a sum into one FMA drops one of the roundings above, and one that associates a
product of three factors the other way - ((o2 d) d), ((lr_step m') / q), as torch's addcmul_ and addcdiv_ do - rounds as often and at
the same magnitudes: both stay within the same bounds.

Statistics.  grad_stats() adds the squares in the order of the kernels: per chunk of CHUNK elements 256 threads; thread i < head takes
element i (head = the elements in front of the gradient's first 16-byte boundary), then thread t the quads t, t + 256, ... element by
element, then one element of the tail; a shuffle tree over each wave of 64, (w0 + w1) + (w2 + w3) over the waves; thread t of the finish
the chunks t, t + 256, ... in order, then the same tree.  The fp64 square of an fp32 value is exact."""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -126
SLACK = 1.0 + 2.0 ** -20
CHUNK = 8192
TPB = 256


def f32(x):
    return np.float32(x)


def bits(a):
    """the bit patterns of an fp32 array, for bit-for-bit comparison"""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scalars(lr, t, betas, eps):
    """-> (lr_step, bc2, o1, b2, o2, eps) as np.float32, from Python doubles in torch's own expressions (_single_tensor_adam)"""
    beta1, beta2 = float(betas[0]), float(betas[1])
    step = float(t)
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return f32(step_size), f32(bias_correction2_sqrt), f32(1 - beta1), f32(beta2), f32(1 - beta2), f32(eps)


def step(p, g, m, v, lr, wd, t, betas=(0.9, 0.999), eps=1e-8, s=None):
    """-> (p', m', v') of one update; p, g, m, v fp32 arrays, t the step count including this step, s None or the fp32 coefficient"""
    assert all(a.dtype == np.float32 for a in (p, g, m, v))
    lr_step, bc2, o1, b2, o2, eps = scalars(lr, t, betas, eps)
    wd = f32(wd)
    with np.errstate(all="ignore"):
        d = g if s is None else f32(s) * g
        d = d if wd == 0 else d + wd * p
        m2 = m + o1 * (d - m)
        v2 = b2 * v + o2 * (d * d)
        q = np.sqrt(v2) / bc2 + eps
        p2 = p - lr_step * (m2 / q)
    assert p2.dtype == m2.dtype == v2.dtype == np.float32
    return p2, m2, v2


def step64(p, g, m, v, lr, wd, t, betas=(0.9, 0.999), eps=1e-8, s=None):
    """the same update in fp64 from the fp32 inputs and the fp32-rounded scalars"""
    lr_step, bc2, o1, b2, o2, eps = (float(x) for x in scalars(lr, t, betas, eps))
    wd = float(f32(wd))
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    d = g if s is None else float(f32(s)) * g
    d = d if wd == 0 else d + wd * p
    m2 = m + o1 * (d - m)
    v2 = b2 * v + o2 * (d * d)
    q = np.sqrt(v2) / bc2 + eps
    return p - lr_step * (m2 / q), m2, v2


def _und(x, err):
    """eta where a product or quotient of exact value x that inherits the error err can leave the normal range, else 0"""
    x = np.abs(x)
    return np.where((x + err < 2.0 ** -125) & ((x != 0) | (err != 0)), ETA, 0.0)


def bounds(p, g, m, v, lr, wd, t, betas=(0.9, 0.999), eps=1e-8, s=None):
    """-> (E_p, E_m, E_v) of the module docstring against step64, fp64 arrays"""
    lr_step, bc2, o1, b2, o2, eps = (float(x) for x in scalars(lr, t, betas, eps))
    wd = float(f32(wd))
    p, g, m, v = (a.astype(np.float64) for a in (p, g, m, v))
    zero = np.zeros_like(p)
    if s is None:
        a, Ea = g, zero
    else:
        a = float(f32(s)) * g
        Ea = U * np.abs(a) + _und(a, zero)
    if wd == 0:
        d, Ed = a, Ea
    else:
        w = wd * p
        Ew = U * np.abs(w) + _und(w, zero)
        d = a + w
        Ed = (1 + U) * (Ea + Ew) + U * np.abs(d)
    e = d - m
    Ee = (1 + U) * Ed + U * np.abs(e)
    f = o1 * e
    Ef = (1 + U) * o1 * Ee + U * np.abs(f) + _und(f, o1 * Ee)
    m2 = m + f
    Em = (1 + U) * Ef + U * np.abs(m2)
    r = d * d
    G = Ed * (2 * np.abs(d) + Ed)
    Er = (1 + U) * G + U * r + _und(r, G)
    x = b2 * v
    Ex = U * np.abs(x) + _und(x, zero)
    y = o2 * r
    Ey = (1 + U) * o2 * Er + U * y + _und(y, o2 * Er)
    v2 = x + y
    Ev = (1 + U) * (Ex + Ey) + U * np.abs(v2)
    z = np.sqrt(v2)
    with np.errstate(all="ignore"):
        S = np.minimum(np.where(z > 0, Ev / np.where(z > 0, z, 1.0), np.inf), np.sqrt(Ev))
    Ez = (1 + U) * S + U * z
    tt = z / bc2
    Et = (1 + U) * Ez / bc2 + U * tt + _und(tt, Ez / bc2)
    q = tt + eps
    Eq = (1 + U) * Et + U * q
    assert (Eq < q).all(), "the denominator's bound reaches the denominator"
    k = m2 / q
    D = (Em + np.abs(k) * Eq) / (q - Eq)
    Ek = (1 + U) * D + U * np.abs(k) + _und(k, D)
    h = lr_step * k
    Eh = (1 + U) * abs(lr_step) * Ek + U * np.abs(h) + _und(h, abs(lr_step) * Ek)
    p2 = p - h
    Ep = (1 + U) * Eh + U * np.abs(p2)
    return Ep * SLACK, Em * SLACK, Ev * SLACK


def check_step(p, g, m, v, lr, wd, t, betas, eps, s, p_new, m_new, v_new, what=""):
    """asserts that (p_new, m_new, v_new) - any fp32 implementation's result for these inputs - lies within the bounds of the fp64
    evaluation; -> the largest |error| / bound of (p', m', v')"""
    want = step64(p, g, m, v, lr, wd, t, betas, eps, s)
    worst = []
    for name, got, w64, E in zip(("p'", "m'", "v'"), (p_new, m_new, v_new), want, bounds(p, g, m, v, lr, wd, t, betas, eps, s)):
        err = np.abs(got.astype(np.float64) - w64)
        with np.errstate(all="ignore"):
            ratio = np.where(err == 0, 0.0, err / E)
        top = float(ratio.max()) if ratio.size else 0.0
        assert top <= 1.0, "%s: %s off by %.3g of its bound" % (what, name, top)
        worst.append(top)
    return tuple(worst)


# ---------------------------------------------------------------------------------------------------------------- statistics and clip
def _tree(a):
    """the fixed tree over 256 per-thread values: a shuffle tree per wave of 64, then (w0 + w1) + (w2 + w3)"""
    a = a.reshape(4, 64).copy()
    off = 32
    while off > 0:
        a[:, :off] += a[:, off:2 * off]
        off >>= 1
    return (a[0, 0] + a[1, 0]) + (a[2, 0] + a[3, 0])


def _chunk_sum(x, head):
    """one chunk's values x (fp64; squares or 0/1 flags) summed in the kernel's order; head: elements in front of the 16-byte boundary"""
    n = x.size
    head = min(head, n)
    s = np.zeros(TPB, np.float64)
    s[:head] += x[:head]
    nq = (n - head) // 4
    quads = x[head:head + 4 * nq].reshape(nq, 4)
    for lo in range(0, nq, TPB):
        part = quads[lo:lo + TPB]
        for k in range(4):
            s[:part.shape[0]] += part[:, k]
    tail = x[head + 4 * nq:]
    s[:tail.size] += tail
    return _tree(s)


def grad_stats(grads, residues=None):
    """-> (sum of g^2, number of non-finite elements) as the kernels add them; grads: fp32 arrays in the call's order, residues: each
    gradient's pointer residue in elements modulo 4 (0 = on a 16-byte boundary; default all 0)"""
    parts = []
    for i, g in enumerate(grads):
        g = np.ascontiguousarray(g, np.float32).ravel()
        res = 0 if residues is None else residues[i] % 4
        with np.errstate(all="ignore"):
            sq = g.astype(np.float64) ** 2
        bad = (~np.isfinite(g)).astype(np.float64)
        for lo in range(0, g.size, CHUNK):        # a chunk keeps the tensor's residue: CHUNK is a multiple of 4
            head = (4 - res) % 4
            with np.errstate(all="ignore"):
                parts.append((_chunk_sum(sq[lo:lo + CHUNK], head), _chunk_sum(bad[lo:lo + CHUNK], head)))
    tot = []
    for k in range(2):
        s = np.zeros(TPB, np.float64)
        with np.errstate(all="ignore"):
            for i, pr in enumerate(parts):        # thread i % 256 adds its partials in ascending order
                s[i % TPB] += pr[k]
            tot.append(_tree(s))
    return float(tot[0]), float(tot[1])


def clip_coef(grad_sq, clip_norm):
    """-> np.float32(clip_norm / max(sqrt(grad_sq), clip_norm)), square root and division in fp64; max() as Python's max(norm,
    clip_norm) in clip_gradient: a NaN norm stays"""
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(grad_sq))
        den = np.float64(clip_norm) if np.float64(clip_norm) > norm else norm
        return np.float32(np.float64(clip_norm) / den)


# ---------------------------------------------------------------------------------------------------------------- fixture
# the single-step cases of tests/golden/adam.npz: name -> (elements, lr, wd, t, betas, eps)
STEP_CASES = {
    "first": (257, 1e-3, 0.0, 1, (0.9, 0.999), 1e-8),
    "first_decay": (257, 1e-3, 1e-4, 1, (0.9, 0.999), 1e-8),
    "second": (257, 1e-3, 1e-4, 2, (0.9, 0.999), 1e-8),
    "late": (257, 1e-2, 0.0, 1000, (0.9, 0.999), 1e-8),
    "late_decay": (257, 1e-2, 1e-4, 1000, (0.9, 0.999), 1e-8),
    "lr_zero": (64, 0.0, 1e-4, 3, (0.9, 0.999), 1e-8),
    "other_betas": (257, 3e-4, 5e-4, 7, (0.5, 0.99), 1e-6),
    "beta1_zero": (64, 1e-3, 0.0, 5, (0.0, 0.999), 1e-8),
}
# the clip cases: name -> (scale of the gradients, clip_norm); the tiny model of CLIP_MODEL plus a 0-d parameter whose gradient is 1
CLIP_CASES = {"clip_below": (0.01, 10.0), "clip_above": (1.0, 0.5), "clip_far_above": (300.0, 0.25), "clip_small_norm": (1.0, 2.0 ** -6)}
CLIP_MODEL = (("fc1.weight", (4, 5)), ("fc1.bias", (4,)), ("fc2.weight", (5, 2)), ("fc2.bias", (5,)))
# the schedule cases: the short ones of sgd_reference.CASES under SOLVER.TYPE = "Adam"
SCHEDULE_CASES = ("short_linear", "short_constant", "short_nowarm")


def adam_cfg(case, **more):
    """the m3d.SolverCfg of a case of sgd_reference.CASES under TYPE = "Adam" (the shipped presets nuclei() / soma() are SGD runs and
    refuse another TYPE: the constructor itself is called)"""
    import m3d
    import sgd_reference as SR
    kw = dict(m3d.SolverCfg.SOMA) if SR.CASES[case][0] == "soma" else {}
    kw.update(SR.CASES[case][1])
    kw.update(more)
    return m3d.SolverCfg(TYPE="Adam", **kw)


def load_case(npz, case):
    """the arrays of one case of tests/golden/adam.npz (tests/golden/gen_adam.py) as a dict without the case prefix"""
    pre = case + "/"
    return {k[len(pre):]: npz[k] for k in npz.files if k.startswith(pre)}
