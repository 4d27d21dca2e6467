"""The f16x2 kernels against fp64, element by element, on inputs that can break a one-scale-per-group cut (tests/f16x2_contract.py):
heavy tails, outliers at 2^12 .. 2^36 x the rest, quiet blocks at 2^-30, inputs at the bound (2^j and the fp32 number below it) and
all-zero inputs, with exact and 2^8-loose bounds.  Every output is finite, within the derived bound E of its fp64 value, and exactly the
shift / bias (or 0) where all its products are zero.  The worst |y^ - y| / E of each call site is printed (pytest -s)."""
import pytest
import torch

import f16x2_contract as K

pytestmark = pytest.mark.gpu

F64 = torch.float64
FAMILIES = ["benign", "heavy", "outlier12", "outlier24", "outlier36", "quiet", "at_bound_pow2", "at_bound_below", "zero"]
WORST = {}


@pytest.fixture(scope="module")
def m3d():
    import m3d as _m
    assert torch.cuda.is_available()
    yield _m
    for site, r in sorted(WORST.items()):
        print("f16x2 contract: worst |y^ - y| / E  %-28s %.3g" % (site, r))
    torch.cuda.empty_cache()


def meets(site, got, y, E, C):
    """got (device) within E of y everywhere, finite, and == y where C == 0"""
    got = got.cpu().to(F64)
    assert got.shape == y.shape
    assert bool(torch.isfinite(got).all()), site
    err = (got - y).abs()
    r = float((err / E.clamp_min(1e-300)).max())
    WORST[site] = max(WORST.get(site, 0.0), r)
    assert bool((err <= E).all()), (site, r)
    z = C == 0
    assert torch.equal(got[z], y[z]), site


# ------------------------------------------------------------------ ZwConv3d (conv3d_zw.hip): both column-block widths, ragged tiles, fused pool
ZW_SHAPES = [(1, 32, 64, 5, 6, 40, False), (1, 16, 40, 3, 10, 20, False), (1, 32, 64, 4, 8, 48, True)]


@pytest.mark.parametrize("shape", ZW_SHAPES, ids=["xb32", "xb16", "pool"])
@pytest.mark.parametrize("name", FAMILIES)
def test_zw_conv_meets_the_contract(m3d, shape, name):
    B, cin, cout, D, H, W, pool = shape
    x, w = K.inputs(name, (B, cin, D, H, W), (cout, cin, 3, 3, 3), cin + W, signed=not pool)
    g = torch.Generator().manual_seed(cout)
    sc, sh = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g)
    conv = m3d.ZwConv3d(w.cuda())
    xc = x.cuda()
    for loose in (False, True):
        bnd = m3d.ZwConv3d.bound_of(xc)
        assert float(bnd.max()) == float(x.abs().max())
        if loose:
            bnd = bnd * 2.0 ** 8
        ib = float(bnd.max())
        if pool:
            got, _ = conv(xc, bnd, scale=sc.cuda(), shift=sh.cuda(), relu=True, pool=True)
            y, E, C = K.zw_contract(x, w, ib, scale=sc, shift=sh, relu=True, pool=True)
        else:
            got, _ = conv(xc, bnd)
            y, E, C = K.zw_contract(x, w, ib)
            meets("ZwConv3d", got, y, E, C)
            got, _ = conv(xc, bnd, scale=sc.cuda(), shift=sh.cuda())
            y, E, C = K.zw_contract(x, w, ib, scale=sc, shift=sh)
        meets("ZwConv3d pool" if pool else "ZwConv3d", got, y, E, C)
        del got


def strip_of(wins, pitch, lead, L):
    cin, n = wins.shape[1], wins.shape[2]
    s = torch.zeros(cin, n, n, L)
    for p in range(wins.shape[0]):
        s[..., lead + p * pitch:lead + p * pitch + n] = wins[p]
    return s


@pytest.mark.parametrize("name", FAMILIES)
def test_zw_strip_meets_the_contract_per_window(m3d, name):
    """ZwConv3d.strip: one scale per window; the windows' insides span 2^30 (a quiet half), their magnitudes 2^-20 .. 2^20"""
    cin, cout, n, P = 32, 32, 10, 5
    pitch, lead, L = m3d.ops.strip_geometry(n, 2, P)
    x, w = K.inputs(name, (P, cin, n, n, n), (cout, cin, 3, 3, 3), 17, signed=True)
    if name not in ("zero",) and not name.startswith("at_bound"):
        x[..., :n // 2] *= 2.0 ** -30
        x *= (2.0 ** torch.linspace(-20, 20, P)).view(P, 1, 1, 1, 1)
    conv = m3d.ops.ZwConv3d(w.cuda())
    s = strip_of(x, pitch, lead, L).cuda().contiguous()
    for loose in (False, True):
        bounds = None
        if loose:
            bounds = torch.zeros(P, 32)
            bounds[:, 0] = x.abs().flatten(1).amax(1) * 2.0 ** 8
            bounds = bounds.cuda()
        got = conv.strip(s, pitch, P, bounds=bounds)
        assert got is not None
        for p in range(P):
            ib = float(x[p].abs().max()) * (2.0 ** 8 if loose else 1.0)
            y, E, C = K.zw_contract(x[p:p + 1], w, ib)
            meets("ZwConv3d.strip", got[..., lead + p * pitch:lead + p * pitch + n].unsqueeze(0), y, E, C)
        del got


def test_zw_strip_beyond_the_sweep_cap(m3d):
    """P = 12289 windows (one more than m3d_prm_strip_absmax takes): without bounds the strip conv returns None (the fp32 strip kernels
    run instead) rather than raising; with the producer's bounds it runs and meets the contract at the windows around the cap"""
    ops = m3d.ops
    cin, cout, n, P = 16, 16, 4, ops.ZwConv3d.STRIP_SWEEP_MAX_PEAKS + 1
    pitch, lead, L = ops.strip_geometry(n, 2, P)
    g = torch.Generator().manual_seed(9)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 0.2
    conv = ops.ZwConv3d(w.cuda())
    sel = [0, 1, P // 2, P - 2, P - 1]
    wins = torch.randn(len(sel), cin, n, n, n, generator=g) * (2.0 ** torch.linspace(-10, 10, len(sel))).view(-1, 1, 1, 1, 1)
    s = torch.zeros(cin, n, n, L, device="cuda")
    for i, p in enumerate(sel):
        s[..., lead + p * pitch:lead + p * pitch + n] = wins[i].cuda()
    assert conv.strip(s, pitch, P) is None
    bounds = torch.zeros(P, 32)
    for i, p in enumerate(sel):
        bounds[p, 0] = float(wins[i].abs().max())
    got = conv.strip(s, pitch, P, bounds=bounds.cuda())
    assert got is not None
    for i, p in enumerate(sel):
        y, E, C = K.zw_contract(wins[i:i + 1], w, float(bounds[p, 0]))
        meets("ZwConv3d.strip", got[..., lead + p * pitch:lead + p * pitch + n].unsqueeze(0), y, E, C)
    del got, s
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ SplitLinearF16 (fc_gemm.hip, F16)
@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("relu", [False, True])
def test_split_linear_f16_meets_the_contract(m3d, name, relu):
    M, N, Kd = 100, 72, 256
    x, w = K.inputs(name, (M, Kd), (N, Kd), Kd + N, signed=True, col=True)
    b = torch.randn(N, generator=torch.Generator().manual_seed(2))
    lin = m3d.ops.SplitLinearF16(w.cuda(), b.cuda())
    xc = x.cuda()
    ys = K.linear_op(x.to(F64), w.to(F64)) + b.to(F64)
    y = torch.relu(ys) if relu else ys
    C, Sa, Sb, n = K.terms(K.linear_op, x, w)
    for mode in ("swept", "exact", "loose"):
        xb = None if mode == "swept" else torch.tensor([float(x.abs().max()) * (2.0 ** 8 if mode == "loose" else 1.0)], device="cuda")
        A = float(x.abs().max()) * (2.0 ** 8 if mode == "loose" else 1.0)
        E = K.bound("fc", Kd, C, Sa, Sb, n, A, float(w.abs().max()), y)
        meets("SplitLinearF16", lin(xc, relu=relu, x_bound=xb), y, E, C)


# ------------------------------------------------------------------ X3Conv3d(f16=True) (conv3d_x3.hip x3f)
@pytest.mark.parametrize("name", FAMILIES)
def test_x3f_norm_conv_meets_the_contract(m3d, name):
    ops = m3d.ops
    cin, cout, D, H, W = 32, 40, 5, 6, 18
    x, w = K.inputs(name, (1, cin, D, H, W), (cout, cin, 3, 3, 3), cin + cout, signed=False)
    xc = x.cuda()
    off = torch.zeros(1, device="cuda") if name.startswith("at_bound") else xc.min().reshape(1)     # X - min X (at the bound: X - 0)
    wr = torch.relu(w)
    a = (x - float(off)).to(torch.float32)                   # the operand the kernel cuts: fl(X - off)
    y = K.conv3d_op(a.to(F64), wr.to(F64))
    C, Sa, Sb, n = K.terms(K.conv3d_op, a, wr)
    c16 = ops.X3Conv3d(w.cuda(), ops.W_RELU, f16=True)
    for loose in (False, True):
        span = float(a.max()) * (2.0 ** 8 if loose else 1.0)
        mx = torch.tensor([K.f32(float(off) + span)], device="cuda")
        A = K.f32(float(mx) - float(off))
        E = K.bound("x3f", cin, C, Sa, Sb, n, A, float(wr.max()), y)
        meets("X3Conv3d(f16)", c16(xc, in_offset=off, in_max=mx), y, E, C)
    # signed weights, no offset: bound = max |x|
    ys = K.conv3d_op(x.to(F64), w.to(F64))
    C, Sa, Sb, n = K.terms(K.conv3d_op, x, w)
    E = K.bound("x3f", cin, C, Sa, Sb, n, float(x.abs().max()), float(w.abs().max()), ys)
    meets("X3Conv3d(f16)", ops.X3Conv3d(w.cuda(), ops.W_PLAIN, f16=True)(xc, in_max=ops.absmax(xc)), ys, E, C)


def test_x3f_norm_conv_gate_at_1e_10_over_a_2_40_span(m3d):
    """N = conv3d(X - min X, relu(W)) with max X - min X = 2^41 and every other operand placed so that N lies around the PostHook's
    1e-10 threshold: outside the band +-E the kernel's N is on the same side of 1e-10 as fp64's (inside it the cut may move N across:
    operands below span 2^-39 vanish)"""
    ops = m3d.ops
    cin, cout, D, H, W = 16, 16, 4, 6, 20
    g = torch.Generator().manual_seed(40)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * 1e-13     # small weights: the band +-E (~ 2^2 sum relu(W)) is narrower than 1e-10
    wr = torch.relu(w)
    t = 1e-10 / float(wr.sum((1, 2, 3, 4)).mean())             # operands near the level where N crosses 1e-10
    x = t * torch.exp(2.0 * torch.randn(1, cin, D, H, W, generator=g))
    x[torch.rand(x.shape, generator=g) < 0.9] = 0.0            # ~40 non-zero taps per output: N on both sides of 1e-10
    x[0, 0, 0, 0, 0] = 2.0 ** 41
    xc = x.cuda()
    off = xc.min().reshape(1)
    assert float(off) == 0.0 and float(x.max()) - float(off) > 2.0 ** 40
    c16 = ops.X3Conv3d(w.cuda(), ops.W_RELU, f16=True)
    got = c16(xc, in_offset=off, in_max=xc.max().reshape(1))
    y = K.conv3d_op(x.to(F64), wr.to(F64))
    C, Sa, Sb, n = K.terms(K.conv3d_op, x, wr)
    E = K.bound("x3f", cin, C, Sa, Sb, n, float(x.max()), float(wr.max()), y)
    meets("X3Conv3d(f16) gate", got, y, E, C)
    gd = got.cpu().to(F64)
    out = (y - 1e-10).abs() > E
    assert int((out & (y < 1e-10) & (y > 0)).sum()) > 0 and int((out & (y > 1e-10)).sum()) > 0      # both sides, outside the band
    assert torch.equal((gd < 1e-10)[out], (y < 1e-10)[out])
    assert bool((gd[y == 0] == 0).all())


def test_norm_conv_gate_at_product_scale_weights_and_span(m3d):
    """Kaiming-scale relu(W) and a span of 10 (a layer's activations): a block of activations at 1.4e-11 gives fp64 N ~ 1.5e-10, above the
    PostHook's 1e-10, while the f16x2 cut's floor (span 2^-39 = 1.8e-11) swallows them - the band +-E of the f16x2 norm conv is wider than
    1e-10 there, so the default PRM path runs the norm convs on the exact bf16x3 cut (PRMEngine x3_f16=False), which puts every N on
    fp64's side of 1e-10 outside its own fp32-class error"""
    ops = m3d.ops
    cin, cout, D, H, W = 16, 16, 6, 8, 20
    g = torch.Generator().manual_seed(41)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) * (2.0 / (cin * 27)) ** 0.5
    wr = torch.relu(w)
    x = torch.zeros(1, cin, D, H, W)
    x[0, 0, 0, 0, 0] = 10.0
    x[:, :, 1:5, 2:7, 6:16] = 1.4e-11 * (1 + 0.1 * torch.rand(1, cin, 4, 5, 10, generator=g))
    xc = x.cuda()
    off = xc.min().reshape(1)
    y = K.conv3d_op(x.to(F64), wr.to(F64))
    C, Sa, Sb, n = K.terms(K.conv3d_op, x, wr)
    E = K.bound("x3f", cin, C, Sa, Sb, n, 10.0, float(wr.max()), y)
    assert bool(((y > 1e-10) & ((y - 1e-10).abs() <= E)).any())            # f16x2: fp64 above the gate, inside the band
    g16 = ops.X3Conv3d(w.cuda(), ops.W_RELU, f16=True)(xc, in_offset=off, in_max=xc.max().reshape(1))
    meets("X3Conv3d(f16) gate", g16, y, E, C)
    flips = int(((g16.cpu().to(F64) < 1e-10) != (y < 1e-10)).sum())
    print("f16x2 norm conv at product scale: %d of %d outputs on the other side of 1e-10" % (flips, y.numel()))
    from m3d.prm import PRMEngine
    import inspect
    assert inspect.signature(PRMEngine.__init__).parameters["x3_f16"].default is False
    gx = ops.X3Conv3d(w.cuda(), ops.W_RELU)(xc, in_offset=off).cpu().to(F64)
    sure = (y - 1e-10).abs() > 1e-4 * y.abs()                      # (beyond the bf16x3 kernel's fp32-class error)
    assert bool((gx[y == 0] == 0).all()) and torch.equal((gx < 1e-10)[sure], (y < 1e-10)[sure])


# ------------------------------------------------------------------ SmallWindowDgrad (prm_small_f16.hip)
def small_case(P, n, cf, cb, seed, name="benign", spread=True):
    g = torch.Generator().manual_seed(seed)
    gn, w = K.inputs(name, (P, cf, n, n, n), (cf, cb, 3, 3, 3), seed, signed=True)
    if spread and name not in ("zero",) and not name.startswith("at_bound"):
        gn = gn * (2.0 ** torch.linspace(-24, 24, P)).view(P, 1, 1, 1, 1)   # each peak starts from its own (1 - y) y
    D, Hh, Ww = 9, 11, 13
    full = torch.randn(cb, D, Hh, Ww, generator=g)
    origins = torch.stack([torch.randint(-n, D, (P,), generator=g), torch.randint(-n, Hh, (P,), generator=g),
                           torch.randint(-n, Ww, (P,), generator=g)], 1).to(torch.int32)
    return gn, w, full, origins


def small_ref(gn, w, full, off, origins, sel):
    """(y, E, C) of the peaks `sel`: dgrad with relu(W) (zero outside the window) x (X - off) inside the volume, 0 outside"""
    wr = torch.relu(w)
    n = gn.shape[2]
    cf, cb = w.shape[0], w.shape[1]
    D, Hh, Ww = full.shape[1:]
    ys, Es, Cs = [], [], []
    r = torch.arange(n)
    for p in sel:
        a = gn[p:p + 1]
        s = K.dgrad_op(a.to(F64), wr.to(F64))[0]
        C, Sa, Sb, nn_ = (t[0] for t in K.terms(K.dgrad_op, a, wr))
        o = origins[p].tolist()
        z, yy, xx = (r + o[0]).view(-1, 1, 1), (r + o[1]).view(1, -1, 1), (r + o[2]).view(1, 1, -1)
        inside = (z >= 0) & (z < D) & (yy >= 0) & (yy < Hh) & (xx >= 0) & (xx < Ww)
        m = torch.zeros(cb, n, n, n, dtype=F64)
        zi, yi, xi = z.clamp(0, D - 1), yy.clamp(0, Hh - 1), xx.clamp(0, Ww - 1)
        m[:] = torch.where(inside, full.to(F64)[:, zi, yi, xi] - float(off), torch.zeros((), dtype=F64))
        y = m * s
        E = K.bound("prm_small", cf, C, Sa, Sb, nn_, float(a.abs().max()), float(wr.max()), y, gain=m.abs())
        C = torch.where(inside, C, torch.zeros((), dtype=F64))
        ys.append(y), Es.append(E), Cs.append(C)
    return torch.stack(ys), torch.stack(Es), torch.stack(Cs)


@pytest.mark.parametrize("name", FAMILIES)
@pytest.mark.parametrize("n", [3, 7])
def test_small_window_dgrad_f16_meets_the_contract(m3d, name, n):
    P, cf, cb = 12, 32, 24
    gn, w, full, origins = small_case(P, n, cf, cb, 5 + n, name)
    op = m3d.SmallWindowDgrad(w.cuda())
    assert op.f16
    fc = full.cuda()
    off = fc.min().reshape(1)
    got = op(gn.cuda(), fc, off, origins.cuda())
    y, E, C = small_ref(gn, w, full, float(off), origins, range(P))
    meets("SmallWindowDgrad(f16)", got, y, E, C)


def test_small_window_dgrad_f16_beyond_the_launch_cap(m3d):
    """P = 65536 3^3 windows (one more than m3d_prm_small_dgrad_f16 takes per launch): the op splits the batch instead of raising; the
    peaks on both sides of the split meet the contract and equal the same peaks run as a batch of their own, bit for bit"""
    P, n, cf, cb = m3d.SmallWindowDgrad.F16_MAX_PEAKS + 1, 3, 16, 16
    gn, w, full, origins = small_case(P, n, cf, cb, 77, spread=False)
    op = m3d.SmallWindowDgrad(w.cuda())
    assert op.f16
    fc = full.cuda()
    off = fc.min().reshape(1)
    got = op(gn.cuda(), fc, off, origins.cuda())
    sel = [0, 1, P - 3, P - 2, P - 1]
    y, E, C = small_ref(gn, w, full, float(off), origins, sel)
    meets("SmallWindowDgrad(f16)", got[sel], y, E, C)
    idx = torch.tensor(sel)
    sub = op(gn[idx].contiguous().cuda(), fc, off, origins[idx].contiguous().cuda())
    assert torch.equal(sub, got[idx.cuda()])
    del got, sub
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ roi_align3d_forward(feat_absmax=) (roi_align3d_fwd_gemm_kernel)
@pytest.mark.parametrize("name", FAMILIES)
def test_roi_align_gemm_meets_the_contract(m3d, name):
    """RoIs whose sub-volumes hold <= 128 voxels (extents 8 .. 20 at scale 1 / 8): one f16x2 GEMM per RoI with the feature map's bound;
    RoIs partly outside the map included"""
    B, Cc, S, H, W = 2, 64, 8, 12, 14
    feat, _ = K.inputs(name, (B, Cc, S, H, W), (1,), 31, signed=True)
    g = torch.Generator().manual_seed(32)
    R = 24
    c = torch.rand(R, 3, generator=g) * torch.tensor([W + 2.0, H + 2.0, S + 2.0]) * 8 - 8
    ext = 8 + 12 * torch.rand(R, 3, generator=g)
    rois = torch.cat([torch.randint(0, B, (R, 1), generator=g).float(), c - ext / 2, c + ext / 2], 1)
    fc, rc = feat.cuda(), rois.cuda()
    for loose in (False, True):
        bnd = m3d.ops.absmax(fc) * (2.0 ** 8 if loose else 1.0)
        got = m3d.roi_align3d_forward(fc, rc, 7, 7, 7, 0.125, 2, feat_absmax=bnd)
        y, E, C = K.roi_contract(feat, rois, 0.125, 2, float(bnd))
        meets("roi_align3d GEMM", got, y, E, C)


# ------------------------------------------------------------------ a stale bound on a refilled out= tensor
def test_out_refill_drops_the_stale_operand_bound(m3d):
    """A bound left on a tensor by the launch that produced it must not survive a later launch that rewrites the tensor through `out=`
    (a ctypes write does not bump `_version`): the next f16x2 conv would scale 1000 x larger values by the old bound and overflow fp16."""
    from m3d.model import DetectorM3D
    ops = m3d.ops
    g = torch.Generator().manual_seed(21)
    x = torch.relu(torch.randn(1, 16, 4, 8, 32, generator=g))
    w1 = torch.randn(32, 16, 3, 3, 3, generator=g) * 0.05
    y, ym = ops.ZwConv3d(w1.cuda())(x.cuda(), ops.ZwConv3d.bound_of(x.cuda()), relu=True)
    y._m3d_bound = (ym, y._version)                           # as the model's layers leave it
    assert DetectorM3D._bound(y) is ym
    v = y._version
    ops.PackedConv3d(w1.cuda() * 1000.0)(x.cuda(), relu=True, out=y)       # 1000 x larger values, written through ctypes
    assert y._version == v and getattr(y, "_m3d_bound", None) is None
    b2 = DetectorM3D._bound(y)
    assert b2 is not ym and float(b2.max()) == float(y.abs().max()) > 100 * float(ym.max())
    w2 = torch.randn(16, 32, 3, 3, 3, generator=g) * 0.05
    z, _ = ops.ZwConv3d(w2.cuda())(y, b2)
    yy = y.cpu()
    ref, E, C = K.zw_contract(yy, w2, float(b2.max()))
    meets("ZwConv3d", z, ref, E, C)
    # the per-window bounds a prepare launch leaves on a strip go the same way
    s = torch.zeros(32, 4, 4, 64, device="cuda")
    s._m3d_peak_max = torch.zeros(8, 32, device="cuda")
    ops.ZwConv3d(torch.randn(32, 32, 3, 3, 3, generator=g).cuda()).strip(torch.rand(32, 4, 4, 64, generator=g).cuda(), 8, 8, out=s)
    assert getattr(s, "_m3d_peak_max", None) is None
