"""GPU: every production instantiation of the four fp32 Winograd conv kernels (csrc/conv3d_wino24.hip, conv3d_wino2.hip, conv3d_stem_wino.hip,
conv3d_wino.hip) against fp64, element by element, over the case table of tests/wino_conv_cases.py (which instantiation a case runs, that
the table covers all of them at ragged tiles, partial chunks and cout tiles, every width residue and every K split, and that the integer
operands are exact, is proved on the CPU by tests/test_wino_conv_cases_host.py).

 (a) exact on integers: integer inputs and weights that are multiples of the kernel's unit make every transformed weight and every
     intermediate an integer below 2^24, so the result must EQUAL the fp64 conv - a transform coefficient off by one, a dropped K chunk of
     a short split-K slice, an epilogue applied per slice, a wrong mask at a ragged quad or a halo element read from the neighbouring row
     all show (the host test seeds exactly these into an emulation and sees them caught);
 (b) the fused pools: pooled values bit-equal to max_pool3d of the exact result, the arg-max by value;
 (c) bounded on random data: the per-element bound of wino_conv_cases.bound (guards the arithmetic at fractional data; the ratio per case
     and the worst per variant are printed, pytest -s)."""
import contextlib
import functools

import pytest
import torch
import torch.nn.functional as F

import wino_conv_cases as T

pytestmark = pytest.mark.gpu

F64 = T.F64
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    for (kernel, variant), r in sorted(WORST.items(), key=str):
        print("winograd conv: worst |got - y| / bound  %-5s %-28s %.4f" % (kernel, variant, r))
    torch.cuda.empty_cache()


@contextlib.contextmanager
def library_for(c):
    """the release library - or, for the stem's 8-plane kernel (which the release library picks from 1024 workgroups on), the tuning
    library with tune_stem = 8"""
    if c.kernel == "stem" and c.variant[1] == 8:
        from m3d import _lib
        with _lib.tuning():
            _lib.set_option("tune_stem", 8)
            yield
    else:
        yield


def conv_of(ops, c, w):
    """the packed conv of the case and the check that the library plans the variant the case names (call inside library_for(c))"""
    shape = (c.batch, c.cin, c.D, c.H, c.W)
    if c.kernel in ("w24", "w22"):
        conv = ops.WinoConv3d(w.cuda(), two_d=True, local=c.kernel == "w22")
        if c.pool:
            assert ops.lib().m3d_conv3d_wino2_family() == 4 and conv.supports_pool(c.W) and c.variant[:3] == (4, 16 if c.W < 48 else 32, 1)
        else:
            assert conv.supports(c.W) and conv.plan(shape) == c.variant[:3], (c, conv.plan(shape))
    elif c.kernel == "stem":
        conv = ops.StemWinoConv3d(w.cuda())
        assert conv.supports(c.W) and conv.plan(shape, pool=c.pool) == c.variant[1], (c, conv.plan(shape, pool=c.pool))
    else:
        conv = ops.WinoConv3d(w.cuda(), two_d=False)
        assert c.variant == T.W23X_RULE(c.cout, c.W, c.pool) and (conv.supports_pool(c.W) if c.pool else conv.supports(c.W))
    return conv


def same(c, got, ref, what):
    """bit-equal to the fp64 reference cast to fp32; on a mismatch, where the wrong elements are: the tile, the row and column inside it and
    the channel block name the path (a K slice cannot be told from the output: the slices of the case are listed)"""
    got, ref = got.cpu().to(torch.float32), ref.to(torch.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = (got != ref).nonzero()
    tx, ty, tz, cot, _ = T.tile_of(c)
    div = (1, 1, tz // 2, ty // 2, tx // 2) if got.shape[2] != c.D or got.shape[4] != c.W else (1, 1, tz, ty, tx)
    first = bad[0].tolist()
    where = {"tiles (x, y, z)": sorted({(int(b[4]) // div[4], int(b[3]) // div[3], int(b[2]) // div[2]) for b in bad[:4096]})[:12],
             "rows in tile": sorted({int(b[3]) % div[3] for b in bad[:4096]}), "columns in tile": sorted({int(b[4]) % div[4] for b in bad[:4096]})[:16],
             "channel blocks of 32": sorted({int(b[1]) // 32 for b in bad[:4096]}), "batch items": sorted({int(b[0]) for b in bad[:4096]})}
    raise AssertionError("%s %s: %d of %d elements differ; first (b, c, z, y, x) %s got %r want %r; last %s; %s; K slices %s"
                         % (T.case_id(c), what, bad.shape[0], ref.numel(), first, float(got[tuple(first)]), float(ref[tuple(first)]),
                            bad[-1].tolist(), where, [len(s) for s in T.slices_of(c)]))


@functools.lru_cache(maxsize=None)
def integer_reference(kernel, shape):
    """operands and fp64 conv of a shape, shared by the cases of that shape and left unchanged"""
    c = next(c for c in T.CASES if c.kernel == kernel and (c.batch, c.cin, c.cout, c.D, c.H, c.W) == shape)
    x, w = T.integer_operands(c)
    return x, w, T.conv64(x, w, T.KSIZE[kernel])


@functools.lru_cache(maxsize=None)
def random_reference(kernel, shape):
    c = next(c for c in T.CASES if c.kernel == kernel and (c.batch, c.cin, c.cout, c.D, c.H, c.W) == shape)
    x, w, scale, shift = T.random_operands(c)
    return x, w, scale, shift, T.conv64(x, w, T.KSIZE[kernel]), T.wino_abs(c, x, w)


def shape_of(c):
    return (c.batch, c.cin, c.cout, c.D, c.H, c.W)


@pytest.mark.parametrize("c", [c for c in T.CASES if not c.pool], ids=T.case_id)
def test_exact_on_integers(ops, c):
    x, w, ref = integer_reference(c.kernel, shape_of(c))
    assert float(x[0, 0, 0, 0, 0]) != 0 and float(x[-1, -1, -1, -1, -1]) != 0           # the shifted first quad, the last masked quad
    scale, shift = T.epilogue_operands(c, negative=c.kernel == "stem")
    ref2 = T.epilogue64(ref, scale, shift)
    with library_for(c):
        conv = conv_of(ops, c, w)
        xd, sd, hd = x.cuda(), scale.cuda(), shift.cuda()
        got = conv(xd)
        same(c, got, ref, "plain")
        got2 = conv(xd, scale=sd, shift=hd, relu=True)              # K split: the reduce kernel applies it
        same(c, got2, ref2, "scale, shift, relu")
        assert torch.equal(conv(xd), got) and torch.equal(conv(xd, scale=sd, shift=hd, relu=True), got2)      # fixed-order split-K


@pytest.mark.parametrize("c", [c for c in T.CASES if c.pool], ids=T.case_id)
def test_fused_pool_exact_on_integers(ops, c):
    """pooled values bit-equal to max_pool3d of the exact conv; the arg-max by value (integer data tie): the un-pooled exact result,
    gathered at it, is the pooled value; the call without arg-max equals the call with it"""
    x, w, plain = integer_reference(c.kernel, shape_of(c))
    scale, shift = T.epilogue_operands(c, negative=c.kernel == "stem")
    full = T.epilogue64(plain, scale, shift)
    with library_for(c):
        conv = conv_of(ops, c, w)
        xd = x.cuda()
        for kw, ref, what in (({}, plain, "plain"), (dict(scale=scale.cuda(), shift=shift.cuda(), relu=True), full, "epilogue")):
            want = F.max_pool3d(ref, 2)
            assert tuple(want.shape[2:]) == (c.D // 2, c.H // 2, c.W // 2)
            if c.argmax:
                got, am = conv.pooled(xd, return_argmax=True, **kw)
                am = am.cpu()
                assert am.dtype == torch.uint8 and int(am.max()) < 8
                same(c, T.pool_gather(ref, am), want, "arg-max " + what)
                same(c, conv.pooled(xd, **kw), want, "pooled without arg-max " + what)
            else:
                got = conv.pooled(xd, **kw)
            same(c, got, want, "pooled " + what)
            assert torch.equal(conv.pooled(xd, **kw), got)


def within(c, what, got, y, bound):
    got = got.cpu().to(F64)
    assert got.shape == y.shape and bool(torch.isfinite(got).all())
    ratio = float(((got - y).abs() / bound.clamp_min(1e-300)).max())
    key = (c.kernel, str(c.variant))
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("winograd conv ratio: %s %s %.4f" % (T.case_id(c), what, ratio))
    assert ratio <= 1.0, (T.case_id(c), what, ratio)


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_bounded_on_random_data(ops, c):
    """N(0,1) inputs, He-scaled weights; the plain conv and the conv with scale / shift / ReLU.  The fused pool: |max a - max b| <= max |a - b|,
    so the pooled result is held to the pooled bound."""
    x, w, scale, shift, y, wabs = random_reference(c.kernel, shape_of(c))
    ye = T.epilogue64(y, scale, shift)
    b1, b2 = T.bound(c, y, wabs), T.bound(c, ye, wabs, scale, shift)
    with library_for(c):
        conv = conv_of(ops, c, w)
        xd, kw = x.cuda(), dict(scale=scale.cuda(), shift=shift.cuda(), relu=True)
        if c.pool:
            within(c, "pooled", conv.pooled(xd), F.max_pool3d(y, 2), F.max_pool3d(b1, 2))
            within(c, "pooled epilogue", conv.pooled(xd, **kw), F.max_pool3d(ye, 2), F.max_pool3d(b2, 2))
        else:
            within(c, "plain", conv(xd), y, b1)
            within(c, "epilogue", conv(xd, **kw), ye, b2)
