"""GPU: the fused SGD step (csrc/sgd.hip) bit for bit against the NumPy restatement of tests/sgd_reference.py - every size at which the
kernel takes another path, aligned and as views 1, 2 and 3 elements into a buffer, between sentinels - its statistics, m3d.Solver on the
reference's recorded schedules, and the stale-pack hazard."""
import numpy as np
import pytest
import torch

import sgd_reference as SR

pytestmark = pytest.mark.gpu

SENT = 64                      # sentinel elements on either side of every tensor
SENT_VALUE = np.float32(-1234.5)


@pytest.fixture(scope="module")
def m3d_gpu():
    import __graft_entry__ as g
    g.build()
    import m3d
    assert torch.cuda.is_available()
    return m3d


class Layout:
    """`count` tensors in one buffer per kind (p, g, m): tensor i lies at elements at[i][kind] .. + n[i], between SENT sentinels; every
    tensor's slot starts on a 16-byte boundary and the tensor `shift` elements into it (shift may differ per kind: the scalar path)."""

    def __init__(self, specs, seed):
        rng = np.random.RandomState(seed)
        self.n = [s[0] for s in specs]
        self.at = []
        pos = 0
        for n, shifts in specs:
            start = pos + SENT
            self.at.append(tuple(start + s for s in shifts))
            pos = (start + 3 + n + SENT + 3) // 4 * 4
        self.total = pos
        self.host = []
        for kind in range(3):
            buf = np.full((self.total,), SENT_VALUE, np.float32)
            for i, n in enumerate(self.n):
                o = self.at[i][kind]
                buf[o:o + n] = (rng.choice([-1.0, 1.0], n) * 2.0 ** rng.uniform(-20, 8, n)).astype(np.float32)
            self.host.append(buf)
        self.lr = [0.01 * (1 + (i % 7) / 8.0) for i in range(len(specs))]
        self.wd = [0.0 if i % 3 == 0 else 1e-4 * (1 + i % 5) for i in range(len(specs))]

    def device(self):
        return [torch.from_numpy(h.copy()).cuda() for h in self.host]

    def views(self, bufs, kind):
        return [bufs[kind][self.at[i][kind]:self.at[i][kind] + n] for i, n in enumerate(self.n)]

    def expect(self, momentum, mscale, with_m):
        """the whole p and m buffers after one step by the restatement (sentinels and gaps untouched)"""
        P, M = self.host[0].copy(), self.host[2].copy()
        for i, n in enumerate(self.n):
            a, b, c = self.at[i]
            p2, m2 = SR.step(self.host[0][a:a + n], self.host[1][b:b + n], self.host[2][c:c + n] if with_m else None, self.lr[i], self.wd[i],
                             momentum, mscale)
            P[a:a + n] = p2
            if with_m:
                M[c:c + n] = m2
        return P, M


def parity_specs(chunk):
    sizes = [0, 1, 3, 4, 5, 63, 255, 4096, 4097, chunk - 1, chunk, chunk + 1, 3 * chunk + 7, 2 ** 22 + 3]
    specs = [(n, (s, s, s)) for n in sizes for s in (0, 1, 2, 3)]
    for _ in range(3):                                            # again with other rates and decays, without the largest
        specs += [(n, (s, s, s)) for n in sizes[:-1] for s in (0, 1, 2, 3)]
    specs += [(n, (0, 0, 0)) for n in (2, 6, 7, 8, 9, 17, 31, 33, 64, 100, 1000, 1023, 1025, 2047, 4095, chunk + 3)]
    specs += [(2 * chunk + 5, (1, 2, 1)), (4099, (0, 0, 3))]      # p and g, p and m at different offsets modulo 16: the scalar path
    assert len(specs) == 230
    return specs


@pytest.fixture(scope="module")
def parity_layout(m3d_gpu):
    return Layout(parity_specs(m3d_gpu.sgd_chunk()), seed=11)


@pytest.mark.parametrize("momentum,mscale,with_m", [(0.9, 1.0, True), (0.9, 0.5, True), (0.0, 1.0, False)])
def test_element_parity(m3d_gpu, parity_layout, momentum, mscale, with_m):
    lay = parity_layout
    bufs = lay.device()
    p, g, m = (lay.views(bufs, k) for k in range(3))
    assert any(t.data_ptr() % 16 == 0 for t in p) and {t.data_ptr() % 16 for t in p} == {0, 4, 8, 12}
    assert (p[-2].data_ptr() - g[-2].data_ptr()) % 16 != 0 and (p[-1].data_ptr() - m[-1].data_ptr()) % 16 != 0
    m3d_gpu.sgd_step(p, g, m if with_m else None, lay.lr, lay.wd, momentum, mscale)
    P, M = lay.expect(momentum, mscale, with_m)
    got_p, got_g, got_m = (b.cpu().numpy() for b in bufs)
    assert np.array_equal(SR.bits(got_g), SR.bits(lay.host[1])), "a gradient or its surroundings were written"
    bad = np.flatnonzero(SR.bits(got_p) != SR.bits(P))
    assert bad.size == 0, "p differs at %d elements, first at buffer index %d" % (bad.size, bad[0])
    bad = np.flatnonzero(SR.bits(got_m) != SR.bits(M))
    assert bad.size == 0, "m differs at %d elements, first at buffer index %d" % (bad.size, bad[0])


def test_nonfinite_gradients(m3d_gpu):
    chunk = m3d_gpu.sgd_chunk()
    lay = Layout([(chunk + 6, (1, 1, 1)), (2 * chunk + 7, (3, 3, 3)), (chunk + 5, (2, 2, 2))], seed=12)
    planted = 0
    for i, n in enumerate(lay.n):
        o = lay.at[i][1]
        for where, value in ((0, np.nan), (n // 2, np.inf), (n - 1, -np.inf)):      # a scalar head, the quads, a scalar tail
            lay.host[1][o + where] = value
            planted += 1
    assert planted == 9 and sum(int((~np.isfinite(lay.host[1][lay.at[i][1]:lay.at[i][1] + n])).sum()) for i, n in enumerate(lay.n)) == 9
    bufs = lay.device()
    p, g, m = (lay.views(bufs, k) for k in range(3))
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    m3d_gpu.sgd_step(p, g, m, lay.lr, lay.wd, 0.9, 1.0, stats)
    P, M = lay.expect(0.9, 1.0, True)
    for got, want in ((bufs[0].cpu().numpy(), P), (bufs[2].cpu().numpy(), M)):
        nan = np.isnan(want)
        assert nan.sum() >= 3 and np.array_equal(np.isnan(got), nan)
        assert np.array_equal(SR.bits(got)[~nan], SR.bits(want)[~nan])
    assert stats[1].item() == 9.0


def test_statistics(m3d_gpu):
    chunk = m3d_gpu.sgd_chunk()
    sizes = [1, 3, 4, 5, 63, 255, 4096, 4097, chunk - 1, chunk, chunk + 1, 3 * chunk + 7]
    specs = [(n, (s, s, s)) for n in sizes for s in (0, 1, 2, 3)] * 2 + [(2 ** 20 + 3, (0, 0, 0))]       # 97 tensors: two launches
    lay = Layout(specs, seed=13)
    N = sum(lay.n)
    want = sum(float((lay.host[1][lay.at[i][1]:lay.at[i][1] + n].astype(np.float64) ** 2).sum()) for i, n in enumerate(lay.n))

    def run(lists=None, empties=0, displace=0, momentum=0.9, drop_m=None):
        bufs = [torch.cat([torch.zeros(displace, device="cuda"), b])[displace:] for b in lay.device()]
        p, g, m = (lay.views(bufs, k) for k in range(3))
        lr, wd = list(lay.lr), list(lay.wd)
        if drop_m is not None:
            m = [None if drop_m(i) else t for i, t in enumerate(m)]
        if empties:      # zero-size tensors add no chunk
            e = torch.zeros(0, device="cuda")
            p, g, m, lr, wd = [e] * empties + p, [e] * empties + g, [e] * empties + m, [0.0] * empties + lr, [0.0] * empties + wd
        out = []
        for lo, hi in (lists or [(0, len(p))]):
            stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
            m3d_gpu.sgd_step(p[lo:hi], g[lo:hi], m[lo:hi], lr[lo:hi], wd[lo:hi], momentum, 1.0, stats)
            out.append(stats.cpu().numpy())
        return out
    a, = run()
    b, = run()
    print("sum g^2: kernel %.17g numpy %.17g, relative difference %.3e (bound %.3e)" % (a[0], want, abs(a[0] - want) / want, N * 2.0 ** -53))
    assert abs(a[0] - want) <= N * 2.0 ** -53 * want
    assert a[1] == 0.0
    assert a.tobytes() == b.tobytes(), "not bit-identical run to run"
    # The defined property (DESIGN, "Solver"): a function of the sizes, order, values and pointer residues modulo 16 of the call's
    # non-empty tensors - not of the addresses, of empty tensors in the list, or of how many launches the call takes.  Tensors without
    # a buffer go through launches of their own: with every other buffer dropped the 97 tensors take about 97 launches instead of 2.
    c, = run(empties=40, displace=260)
    assert a.tobytes() == c.tobytes(), "the result depends on the addresses or on empty tensors"
    d, = run(momentum=0.0, drop_m=lambda i: i % 2 == 1)
    assert a.tobytes() == d.tobytes(), "the result depends on where the call's launches split"
    # two calls over the halves of the list: each is a call of its own with its own finish; their sum meets the same bound
    h1, h2 = run([(0, 50), (50, len(specs))])
    assert abs((h1[0] + h2[0]) - want) <= N * 2.0 ** -53 * want and h1[1] == h2[1] == 0.0
    # nothing to add up: zeros, not what the buffer held
    stats = torch.full((2,), -1.0, dtype=torch.float64, device="cuda")
    m3d_gpu.sgd_step([], [], [], [], [], 0.9, 1.0, stats)
    assert stats.cpu().tolist() == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------------------------- Solver
class _Leaf(torch.nn.Module):
    def __init__(self, weight, bias):
        super().__init__()
        self.weight, self.bias = torch.nn.Parameter(weight), torch.nn.Parameter(bias)


def tiny_module(arrays):
    """the fixture's model (sgd_reference.MODEL) as a module on the device"""
    shapes = dict(SR.MODEL)
    m = torch.nn.Module()
    for leaf in ("fc1", "fc2"):
        w, b = (torch.tensor(arrays["init.%s.%s" % (leaf, k)], dtype=torch.float32) if arrays is not None else
                torch.zeros(shapes["%s.%s" % (leaf, k)]) for k in ("weight", "bias"))
        m.add_module(leaf, _Leaf(w, b))
    return m.cuda()


GROUP = {name: (1 if "bias" in name else 0) for name, _ in SR.MODEL}


@pytest.mark.parametrize("case", ["short_linear", "short_resume"])
def test_solver_against_restatement(m3d_gpu, golden, tmp_path, case):
    m3d = m3d_gpu
    a = SR.load_case(golden("solver"), case)
    cfg = SR.solver_cfg(case)
    resume_after = SR.CASES[case][2]
    model = tiny_module(a)
    solver = m3d.Solver(model.named_parameters(), cfg)
    p = {n: a["init." + n].astype(np.float32) for n, _ in SR.MODEL}
    m = {n: np.zeros_like(p[n]) for n in p}
    index = {n: i for i, n in enumerate([n for n, _ in SR.MODEL if GROUP[n] == 0] + [n for n, _ in SR.MODEL if GROUP[n] == 1])}
    step = 0
    while step < cfg.MAX_ITER:
        solver.begin_step(step)
        assert (solver.param_groups[0]["lr"], solver.param_groups[1]["lr"]) == tuple(a["rates"][step])
        factor = solver.mscale
        solver.zero_grad()
        for n, q in model.named_parameters():
            q.grad = torch.from_numpy(a["grad." + n][step].copy()).cuda()
        solver.step()
        assert solver.mscale == 1.0
        sd = solver.state_dict()
        for n, q in model.named_parameters():
            g = solver.param_groups[GROUP[n]]
            p[n], m[n] = SR.step(p[n], a["grad." + n][step], m[n], g["lr"], g["weight_decay"], g["momentum"], factor)
            assert np.array_equal(SR.bits(q.detach().cpu().numpy()), SR.bits(p[n])), (case, step, n)
            assert np.array_equal(SR.bits(sd["state"][index[n]]["momentum_buffer"].cpu().numpy()), SR.bits(m[n])), (case, step, n)
        if step == resume_after:         # through a real file into a fresh model and solver
            path = m3d.save_ckpt(str(tmp_path), step, model, solver)
            model = tiny_module(None)
            solver = m3d.Solver(model.named_parameters(), cfg)
            assert m3d.load_ckpt(path, model, solver) == step + 1
        step += 1
    # the straight run and the resumed one end on the same bits: both equal the restatement, whose state never left the host; and the
    # fp32 run ends near the reference's fp64 one
    for n, q in model.named_parameters():
        assert np.abs(q.detach().cpu().numpy().astype(np.float64) - a["p." + n][-1]).max() <= 1e-5


def test_stale_packs(m3d_gpu):
    """The update writes through raw pointers: without invalidate_packs() in Solver.step the cached conv and linear packs would still
    hold the old weights."""
    m3d = m3d_gpu
    import m3d.compat
    torch.manual_seed(5)
    lin = torch.nn.Linear(64, 64).cuda()
    conv = torch.nn.Conv3d(16, 16, 3, padding=1).cuda()
    x = torch.randn(8, 64, device="cuda")
    v = torch.randn(1, 16, 8, 8, 24, device="cuda")
    m3d.compat.install()
    try:
        y0, z0 = lin(x).detach(), conv(v).detach()
        assert m3d.compat._lin_cache and m3d.compat._pack_cache, "the forward went through libm3d and cached its packs"
        bias_y, bias_z = lin.bias.detach()[None, :].expand_as(y0), conv.bias.detach()[None, :, None, None, None].expand_as(z0)
        top_y, top_z = y0.abs().max().item(), z0.abs().max().item()
        assert (y0 - bias_y).abs().max().item() > 0.5 * top_y and (z0 - bias_z).abs().max().item() > 0.5 * top_z
        cfg = m3d.SolverCfg.nuclei(BASE_LR=1.0, MOMENTUM=0.0, WEIGHT_DECAY=0.0, WARM_UP_ITERS=0)
        solver = m3d.Solver([("lin.weight", lin.weight), ("conv.weight", conv.weight)], cfg)
        assert solver.begin_step(0) == 1.0
        for q in (lin.weight, conv.weight):
            q.grad = q.detach().clone()
        solver.step()
        assert lin.weight.abs().max().item() == 0.0 and conv.weight.abs().max().item() == 0.0
        y1, z1 = lin(x).detach(), conv(v).detach()
        assert (y1 - bias_y).abs().max().item() <= 1e-4 * top_y
        assert (z1 - bias_z).abs().max().item() <= 1e-4 * top_z
    finally:
        m3d.compat.uninstall_conv3d()
        m3d.compat.uninstall_linear()
