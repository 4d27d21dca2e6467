"""GPU: the fused Adam step, the clip coefficient and the scaled SGD step (csrc/adam.hip, csrc/sgd.hip) bit for bit against the NumPy
restatements of tests/adam_reference.py and tests/sgd_reference.py - every size at which the kernels take another path, as views 0 to 3
elements off a 16-byte boundary, between sentinels, one tensor with four different residues (the element-by-element path), 65 tensors
(two launches) - the statistics, m3d.Solver under TYPE="Adam" with and without CLIP_NORM, the stale-pack hazard and graph capture.
Denormal moments are left out: |g| lies in 2^[-20, 4] or is 0, m likewise, v is a square of such a value or 0."""
import numpy as np
import pytest
import torch

import adam_reference as AR
import sgd_reference as SR

pytestmark = pytest.mark.gpu

SENT = 64                      # sentinel elements on either side of every tensor
SENT_VALUE = np.float32(-1234.5)
BETAS, EPS = (0.9, 0.999), 1e-8
P, G, M, V = range(4)


@pytest.fixture(scope="module")
def m3d_gpu():
    import __graft_entry__ as g
    g.build()
    import m3d
    assert torch.cuda.is_available()
    assert m3d.sgd_chunk() == AR.CHUNK
    return m3d


def mags(rng, n, lo, hi):
    return (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(lo, hi, n)).astype(np.float32)


class Layout:
    """`count` tensors in one buffer per kind (p, g, m, v): tensor i lies at elements at[i][kind] .. + n[i], between SENT sentinels; every
    tensor's slot starts on a 16-byte boundary and the tensor `shift` elements into it (shifts that differ per kind: the scalar path)."""

    def __init__(self, specs, seed):
        rng = np.random.RandomState(seed)
        self.n = [s[0] for s in specs]
        self.shift = [s[1] for s in specs]
        self.at = []
        pos = 0
        for n, shifts in specs:
            start = pos + SENT
            self.at.append(tuple(start + s for s in shifts))
            pos = (start + 3 + n + SENT + 3) // 4 * 4
        self.total = pos
        self.host = [np.full((self.total,), SENT_VALUE, np.float32) for _ in range(4)]
        for i, n in enumerate(self.n):
            p, g, m = mags(rng, n, -6, 3), mags(rng, n, -20, 4), mags(rng, n, -20, 4)
            v = mags(rng, n, -20, 4) ** 2
            g[::7] = 0.0                       # exact zeros among the gradients
            m[3::11], v[5::13] = 0.0, 0.0
            lo = n // 3                        # a block with g = 0 and v = 0
            g[lo:lo + 40], v[lo:lo + 40] = 0.0, 0.0
            for kind, x in zip(range(4), (p, g, m, v)):
                o = self.at[i][kind]
                self.host[kind][o:o + n] = x
        k = len(specs)
        self.lr = [0.0 if i % 9 == 4 else 1e-3 * (1 + (i % 7) / 8.0) for i in range(k)]
        self.wd = [0.0 if i % 2 == 0 else 1e-4 for i in range(k)]

    def device(self, kinds=range(4)):
        return [torch.from_numpy(self.host[k].copy()).cuda() for k in kinds]

    def views(self, buf, kind):
        return [buf[self.at[i][kind]:self.at[i][kind] + n] for i, n in enumerate(self.n)]

    def part(self, kind, i, host=None):
        o = self.at[i][kind]
        return (self.host if host is None else host)[kind][o:o + self.n[i]]

    def grads(self):
        return [self.part(G, i) for i in range(len(self.n))]

    def residues(self):
        return [s[G] for s in self.shift]


def specs_of(chunk):
    sizes = [0, 1, 3, 4, 5, chunk - 1, chunk, chunk + 1, 2 * chunk + 7]
    specs = [(n, (s, s, s, s)) for n in sizes for s in (0, 1, 2, 3)]
    specs += [(n, (s, s, s, s)) for n in sizes[:7] for s in (0, 1, 2, 3)]          # again with other rates and decays
    specs += [(2 * chunk + 5, (1, 2, 3, 0))]                                       # four residues: element by element
    assert len(specs) == 65                                                        # two launches
    return specs


@pytest.fixture(scope="module")
def layout(m3d_gpu):
    return Layout(specs_of(m3d_gpu.sgd_chunk()), seed=21)


def assert_bits(got, want, what):
    bad = np.flatnonzero(AR.bits(got) != AR.bits(want))
    assert bad.size == 0, "%s differs at %d elements, first at buffer index %d" % (what, bad.size, bad[0])


# ---------------------------------------------------------------------------------------------------------------- the update
@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("s", [None, 0.3125, 0.0707734301686287])
def test_element_parity(m3d_gpu, layout, t, s):
    lay = layout
    host = [h.copy() for h in lay.host]
    if t == 1:                                 # torch's first step starts from zero moments
        for i, n in enumerate(lay.n):
            lay.part(M, i, host)[:] = 0.0
            lay.part(V, i, host)[:] = 0.0
    bufs = [torch.from_numpy(h.copy()).cuda() for h in host]
    p, g, m, v = (lay.views(bufs[k], k) for k in range(4))
    assert {x.data_ptr() % 16 for x in p} == {0, 4, 8, 12}
    assert len({x[-1].data_ptr() % 16 for x in (p, g, m, v)}) == 4
    assert 0.0 in lay.lr and {0.0, 1e-4} == set(lay.wd)
    gscale = None if s is None else torch.tensor([s], dtype=torch.float32, device="cuda")
    steps = [t] * len(p)
    stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    m3d_gpu.adam_step(p, g, m, v, lay.lr, lay.wd, steps, BETAS, EPS, stats=stats, gscale=gscale)
    want = [h.copy() for h in host]
    for i, n in enumerate(lay.n):
        args = [lay.part(k, i, host) for k in range(4)]
        p2, m2, v2 = AR.step(*args, lay.lr[i], lay.wd[i], t, BETAS, EPS, s)
        blk = (args[G] == 0) & (args[V] == 0)
        assert n < 100 or blk.sum() >= 40
        if s is None and lay.wd[i] == 0:       # g = 0, v = 0: v' = 0, and with lr = 0 also p' = p; m' as the restatement rounds it
            o1 = np.float32(1 - BETAS[0])
            assert not v2[blk].any() and np.array_equal(AR.bits(m2[blk]), AR.bits(args[M][blk] + o1 * (np.float32(0) - args[M][blk])))
        if lay.lr[i] == 0:
            assert np.array_equal(AR.bits(p2), AR.bits(args[P]))
        for kind, x in ((P, p2), (M, m2), (V, v2)):
            lay.part(kind, i, want)[:] = x
    got = [b.cpu().numpy() for b in bufs]
    assert np.array_equal(AR.bits(got[G]), AR.bits(host[G])), "a gradient or its surroundings were written"
    for kind, name in ((P, "p"), (M, "m"), (V, "v")):
        assert np.isfinite(want[kind]).all()
        assert_bits(got[kind], want[kind], name)
    # the statistics are those of the raw gradients, in the order the restatement adds them
    gsq, bad = AR.grad_stats(lay.grads(), lay.residues())
    assert stats.cpu().tolist() == [gsq, bad] and bad == 0.0


def test_five_steps_one_parameter_sits_out(m3d_gpu):
    """m3d.Solver(TYPE="Adam") over five steps of fixed gradients, with and without CLIP_NORM; fc2.weight has no gradient on steps 2
    and 3: its step count lags and its p, m and v are untouched there"""
    m3d = m3d_gpu
    chunk = m3d.sgd_chunk()
    shapes = (("fc1.weight", (chunk // 4 + 3, 5)), ("fc1.bias", (5,)), ("fc2.weight", (5, 2)), ("fc2.bias", (5,)))
    order = ["fc1.weight", "fc2.weight", "fc1.bias", "fc2.bias"]           # the solver's: non-bias, then bias
    rng = np.random.RandomState(31)
    init = {n: mags(rng, int(np.prod(s)), -6, 1).reshape(s) for n, s in shapes}
    grads = [{n: mags(rng, int(np.prod(s)), -12, 2).reshape(s) for n, s in shapes} for _ in range(5)]
    for clip in (None, 0.75):
        params = {n: torch.nn.Parameter(torch.from_numpy(init[n].copy()).cuda()) for n, _ in shapes}
        cfg = m3d.SolverCfg(TYPE="Adam", BASE_LR=1e-3, WARM_UP_ITERS=3, STEPS=(0, 4), MAX_ITER=5, CLIP_NORM=clip)
        solver = m3d.Solver(list(params.items()), cfg, stats=True)
        p = {n: init[n].copy() for n in init}
        m = {n: np.zeros_like(init[n]) for n in init}
        v = {n: np.zeros_like(init[n]) for n in init}
        count = {n: 0 for n in init}
        for step in range(5):
            solver.begin_step(step)
            assert solver.mscale == 1.0
            solver.zero_grad()
            live = [n for n in order if not (n == "fc2.weight" and step in (1, 2))]
            for n in live:
                params[n].grad = torch.from_numpy(grads[step][n].copy()).cuda()
            solver.step()
            gsq, bad = AR.grad_stats([grads[step][n] for n in live])
            assert (solver.grad_sq.item(), solver.nonfinite.item()) == (gsq, bad)
            s = None
            if clip is not None:
                s = AR.clip_coef(gsq, clip)
                assert AR.bits(solver.clip_coef.cpu().numpy()) == AR.bits(s) and (s < 1.0) == (np.sqrt(gsq) > clip)
            sd = solver.state_dict()
            for i, n in enumerate(order):
                g = solver.param_groups[0 if "bias" not in n else 1]
                if n in live:
                    count[n] += 1
                    p[n], m[n], v[n] = AR.step(p[n], grads[step][n], m[n], v[n], g["lr"], g["weight_decay"], count[n], BETAS, EPS, s)
                assert np.array_equal(AR.bits(params[n].detach().cpu().numpy()), AR.bits(p[n])), (clip, step, n)
                if count[n]:
                    st = sd["state"][i]
                    assert float(st["step"]) == count[n]
                    assert np.array_equal(AR.bits(st["exp_avg"].cpu().numpy()), AR.bits(m[n])), (clip, step, n)
                    assert np.array_equal(AR.bits(st["exp_avg_sq"].cpu().numpy()), AR.bits(v[n])), (clip, step, n)
                else:
                    assert i not in sd["state"]
        assert count == {"fc1.weight": 5, "fc2.weight": 3, "fc1.bias": 5, "fc2.bias": 5}


# ---------------------------------------------------------------------------------------------------------------- scaled SGD
@pytest.mark.parametrize("momentum,mscale,with_m", [(0.9, 1.0, True), (0.9, 0.5, True), (0.0, 1.0, False)])
def test_scaled_sgd(m3d_gpu, layout, momentum, mscale, with_m):
    lay = layout
    lr = [0.01 * (1 + (i % 7) / 8.0) for i in range(len(lay.n))]

    def run(fn, **kw):
        bufs = lay.device(range(3))
        p, g, m = (lay.views(bufs[k], k) for k in range(3))
        stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        fn(p, g, m if with_m else None, lr, lay.wd, momentum, mscale, stats, **kw)
        return [b.cpu().numpy() for b in bufs], stats.cpu().numpy()
    plain, stats0 = run(m3d_gpu.sgd_step)
    null, stats1 = run(m3d_gpu.sgd_step_scaled, gscale=None)
    for a, b, name in zip(plain, null, "pgm"):
        assert_bits(b, a, name + " without a coefficient")
    assert stats0.tobytes() == stats1.tobytes()
    s = np.float32(0.0707734301686287)
    got, stats2 = run(m3d_gpu.sgd_step_scaled, gscale=torch.tensor([float(s)], dtype=torch.float32, device="cuda"))
    assert stats2.tobytes() == stats0.tobytes(), "the statistics are those of the raw gradients"
    want = [h.copy() for h in lay.host[:3]]
    for i, n in enumerate(lay.n):
        p2, m2 = SR.step(lay.part(P, i), s * lay.part(G, i), lay.part(M, i) if with_m else None, lr[i], lay.wd[i], momentum, mscale)
        lay.part(P, i, want)[:] = p2
        if with_m:
            lay.part(M, i, want)[:] = m2
    for a, b, name in zip(got, want, "pgm"):
        assert_bits(a, b, name + " with a coefficient")


# ---------------------------------------------------------------------------------------------------------------- the coefficient
def test_clip_coefficient_and_statistics(m3d_gpu, layout):
    lay = layout
    bufs = lay.device()
    g = lay.views(bufs[G], G)
    gsq, bad = AR.grad_stats(lay.grads(), lay.residues())
    norm = float(np.sqrt(gsq))

    def coef_of(clip_norm, grads=g):
        stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
        coef = torch.full((1,), -1.0, dtype=torch.float32, device="cuda")
        m3d_gpu.grad_clip_coef(grads, clip_norm, stats, coef)
        return stats.cpu().numpy(), coef.cpu().numpy()
    below, c_below = coef_of(2.0 * norm)
    above, c_above = coef_of(norm / 7.0)
    again, c_again = coef_of(norm / 7.0)
    assert below.tolist() == above.tolist() == [gsq, bad] and bad == 0.0
    assert c_below[0] == np.float32(1.0)
    assert AR.bits(c_above) == AR.bits(AR.clip_coef(gsq, norm / 7.0)) and 0.14 < c_above[0] < 0.15
    assert above.tobytes() == again.tobytes() and c_above.tobytes() == c_again.tobytes(), "not bit-identical run to run"
    assert np.array_equal(AR.bits(bufs[G].cpu().numpy()), AR.bits(lay.host[G])), "a gradient or its surroundings were written"
    # the same gradient list through m3d_sgd_step (p and m at the gradient's residue: its 16-byte path) leaves the same two numbers
    gp = [lay.at[i][G] for i in range(len(lay.n))]
    pb, mb = (torch.zeros(lay.total, device="cuda") for _ in range(2))
    p, m = ([b[o:o + n] for o, n in zip(gp, lay.n)] for b in (pb, mb))
    sgd = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    m3d_gpu.sgd_step(p, g, m, lay.lr, lay.wd, 0.9, 1.0, sgd)
    assert sgd.cpu().numpy().tobytes() == above.tobytes()
    # ... and through m3d_adam_step, also for the tensor that it updates element by element
    rest = lay.device()
    adam = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    m3d_gpu.adam_step(lay.views(rest[P], P), lay.views(rest[G], G), lay.views(rest[M], M), lay.views(rest[V], V), lay.lr, lay.wd,
                      [2] * len(lay.n), BETAS, EPS, stats=adam)
    assert adam.cpu().numpy().tobytes() == above.tobytes()
    # an empty list: zeros and a coefficient of 1
    s0, c0 = coef_of(1.0, [])
    assert s0.tolist() == [0.0, 0.0] and c0[0] == np.float32(1.0)


def test_nan_gradient(m3d_gpu, layout):
    lay = layout
    bufs = lay.device()
    big = max(range(len(lay.n)), key=lambda i: lay.n[i])
    bufs[G][lay.at[big][G] + lay.n[big] // 2] = float("nan")
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    coef = torch.zeros(1, dtype=torch.float32, device="cuda")
    m3d_gpu.grad_clip_coef(lay.views(bufs[G], G), 1.0, stats, coef)
    assert np.isnan(coef.item()) and np.isnan(stats[0].item()) and stats[1].item() == 1.0
    p, g, m, v = (lay.views(bufs[k], k) for k in range(4))
    m3d_gpu.adam_step(p, g, m, v, lay.lr, lay.wd, [3] * len(p), BETAS, EPS, gscale=coef)
    moved = [i for i, n in enumerate(lay.n) if n > 0]
    assert all(torch.isnan(m[i]).all() and torch.isnan(v[i]).all() for i in moved), "the step is non-finite: nonfinite is the guard"
    assert all(torch.isnan(p[i]).all() for i in moved if lay.lr[i] != 0)
    for k in (P, M, V):       # and nothing outside the tensors
        outside = np.ones(lay.total, bool)
        for i, n in enumerate(lay.n):
            outside[lay.at[i][k]:lay.at[i][k] + n] = False
        assert (bufs[k].cpu().numpy()[outside] == SENT_VALUE).all()


# ---------------------------------------------------------------------------------------------------------------- Solver
def test_stale_packs(m3d_gpu):
    """The test_stale_packs of the SGD solver under Adam.  From zero moments at t = 1 and without decay the step h = lr_step (m' / q)
    does not depend on the weights, so weights set to the restatement's h land exactly on 0; the next compat forward must see that."""
    m3d = m3d_gpu
    import m3d.compat
    torch.manual_seed(6)
    lin = torch.nn.Linear(64, 64).cuda()
    conv = torch.nn.Conv3d(16, 16, 3, padding=1).cuda()
    x = torch.randn(8, 64, device="cuda")
    vol = torch.randn(1, 16, 8, 8, 24, device="cuda")
    rng = np.random.RandomState(7)
    grads = {}
    with torch.no_grad():
        for name, q in (("lin", lin.weight), ("conv", conv.weight)):
            g = mags(rng, q.numel(), -8, 2).reshape(tuple(q.shape))
            zero = np.zeros_like(g)
            h = -AR.step(zero, g, zero, zero, 1.0, 0.0, 1, BETAS, EPS)[0]
            assert 0.99 < np.abs(h).min() and np.abs(h).max() < 1.01
            q.copy_(torch.from_numpy(h))
            grads[name] = torch.from_numpy(g).cuda()
    m3d.compat.install()
    try:
        y0, z0 = lin(x).detach(), conv(vol).detach()
        assert m3d.compat._lin_cache and m3d.compat._pack_cache, "the forward went through libm3d and cached its packs"
        bias_y, bias_z = lin.bias.detach()[None, :].expand_as(y0), conv.bias.detach()[None, :, None, None, None].expand_as(z0)
        top_y, top_z = y0.abs().max().item(), z0.abs().max().item()
        assert (y0 - bias_y).abs().max().item() > 0.5 * top_y and (z0 - bias_z).abs().max().item() > 0.5 * top_z
        cfg = m3d.SolverCfg(TYPE="Adam", BASE_LR=1.0, WEIGHT_DECAY=0.0, WARM_UP_ITERS=0)
        solver = m3d.Solver([("lin.weight", lin.weight), ("conv.weight", conv.weight)], cfg)
        assert solver.begin_step(0) == 1.0
        lin.weight.grad, conv.weight.grad = grads["lin"], grads["conv"]
        solver.step()
        assert lin.weight.abs().max().item() == 0.0 and conv.weight.abs().max().item() == 0.0
        y1, z1 = lin(x).detach(), conv(vol).detach()
        assert (y1 - bias_y).abs().max().item() <= 1e-4 * top_y
        assert (z1 - bias_z).abs().max().item() <= 1e-4 * top_z
    finally:
        m3d.compat.uninstall_conv3d()
        m3d.compat.uninstall_linear()


@pytest.mark.parametrize("kind", ["Adam", "SGD"])
def test_clipped_step_in_a_graph(m3d_gpu, kind):
    """one clipped Solver.step() captured and replayed once gives the bits of the eager step: no host read, allocation that the capture
    forbids, or copy; a single stream, no parallel branches"""
    m3d = m3d_gpu
    chunk = m3d.sgd_chunk()
    rng = np.random.RandomState(41)
    shapes = (("a.weight", (chunk + 9,)), ("a.bias", (7,)), ("b.weight", (3, 5)))
    init = {n: mags(rng, int(np.prod(s)), -6, 1).reshape(s) for n, s in shapes}
    grad = {n: mags(rng, int(np.prod(s)), -8, 2).reshape(s) for n, s in shapes}
    cfg = m3d.SolverCfg(TYPE=kind, CLIP_NORM=0.5, WARM_UP_ITERS=0)

    def make():
        params = [(n, torch.nn.Parameter(torch.from_numpy(init[n].copy()).cuda())) for n, _ in shapes]
        solver = m3d.Solver(params, cfg)
        solver.begin_step(0)
        for n, q in params:
            q.grad = torch.from_numpy(grad[n].copy()).cuda()
        return params, solver
    eager_params, eager = make()
    eager.step()
    torch.cuda.synchronize()
    assert 0.0 < eager.clip_coef.item() < 1.0
    params, solver = make()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        solver.step()
    torch.cuda.synchronize()
    for (n, q), (_, e) in zip(params, eager_params):
        assert np.array_equal(AR.bits(q.detach().cpu().numpy()), AR.bits(init[n])), "the capture ran nothing"
    g.replay()
    torch.cuda.synchronize()
    for (n, q), (_, e) in zip(params, eager_params):
        assert np.array_equal(AR.bits(q.detach().cpu().numpy()), AR.bits(e.detach().cpu().numpy())), n
    assert AR.bits(solver.clip_coef.cpu().numpy()) == AR.bits(eager.clip_coef.cpu().numpy())
    assert solver.grad_sq.item() == eager.grad_sq.item() and solver.nonfinite.item() == 0.0
    a, b = solver.state_dict()["state"], eager.state_dict()["state"]
    assert sorted(a) == sorted(b) == [0, 1, 2]
    for i in a:
        for k in a[i]:
            assert torch.equal(a[i][k].cpu(), b[i][k].cpu()), (i, k)
