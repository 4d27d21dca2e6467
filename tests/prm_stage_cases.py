"""Case tables, fp64 references, error bounds and layout helpers for the stages of the peak-response back-propagation (csrc/prm.hip,
prm_stem_mfma.hip, prm_small.hip and the PreHook epilogue of the windowed direct conv).  No tests live here:
tests/test_prm_stage_cases_host.py proves on the CPU that the references compose to oracle.prm_backward, that the table reaches every
kernel the two host queries name (m3d_prm_prepare_plan, m3d_prm_stem_dgrad_plan) and that the exact comparison catches mutants;
tests/test_gpu_prm_stages.py runs the table on the GPU.

References.  Written from lib/prm/peak_backprop_3d.py:8-44 and lib/prm/peak_response_mapping_3d.py:157-172 on WHOLE maps: a window is
`place`d into a zero map of the layer at its virtual origin, the layer's rule is applied to the map, and the result window is `crop`ped
out at the new origin (zero where it sticks out).  None of the kernels' index arithmetic appears.  Decisions are the fp32 run's: eps =
float32(1e-10) compared with the fp32 norm (`norm < eps` -> 0, so a large negative norm gives 0 too, else g / (|norm| + eps)), the ReLU
mask is xnext > 0, the denominator |norm| + eps is that run's one fp32 add (`denominator`); everything else is fp64 (`dt`; the host test also runs the references in fp32 as an independent evaluation).

Two comparisons per case (tests/test_gpu_prm_stages.py):
 (a) exact: integer-valued gradients, weights, scales and (X - off), divisors that are exactly representable (norm 0, negative, below
     eps, or a power of two >= 2^-9, for which |n| + eps == |n| in fp32; den 0 or 1), every partial sum below 2^24: any summation order
     is exact and the result must EQUAL the fp64 reference bit for bit.  (For the sums the sign of a zero is not compared: -0 + 0 depends
     on the first addend.)
 (b) bounded: random fp32 data, magnitudes spread over decades per peak, cut edges sprinkled into norm and xnext (NORM_EDGES,
     XNEXT_EDGES).  u = 2^-24.
       pointwise stages  |got - y| <= k u |y|, zeros exact, signs equal.  k = the fp32 operations on the path; the divide counts 3: a
                         correctly rounded divide is 1, a reciprocal-and-multiply expansion without the final correction is allowed
                         2.5 ulp by the OpenCL/HIP accuracy tables, and the bound must not depend on the compiler's choice.
                           seed      9 = (1 - y), * y, |n| + eps, divide (3), relu(w) * gn, h - off, the product
                           prepare   4 + 2 [up_off: xnext - off, multiply] + 1 [scale] = |n| + eps, divide (3), ...
                           den_pool  1 = |n| + eps
                           scatter   3 = the divide
       sums              |got - y| <= (C3 n_acc + k_g) u Cabs |X - off| + 2 u |y|  (the clamped stems: 2 u Cabs |X - off|),  Cabs = sum |w| |G| in fp64, n_acc = terms + 3 (any
                         summation order), C3 = 2 as in tests/f16x2_contract.py (an accumulate that truncates), k_g = the pointwise
                         operations that produce G inside the same kernel (fused stem: 4 + 2 [up_off] + 1 [scale]; else 0), 2 = the
                         subtraction X - off and the PreHook product.
                           windowed conv / small GEMM   terms = 27 * channels of G
                           stem (both forms)            terms = 125 * channels of G
       per-peak sums     |got - sum y| <= sum of the element bounds + a u sum |got|, a = the adds a value passes in window_sums_kernel:
                         float4 path (w3 % 4 == 0): 2 inside the quad + ceil(w3 / 4096) into the thread's accumulator + 10 tree levels;
                         scalar path: ceil(w3 / 1024) + 10.

Largest measured |got - y| / bound per stage (MI355X; printed by the GPU tests, pytest -s; the bounds are not tuned to them; every exact
comparison held bit for bit):
    seed 0.2994     den_pool 0 (its one operation is the reference's own fp32 add)     scatter 0.3247
    prepare: element 0.3688   quad<8> 0.4020   quad<16> 0.4811   quad<32> 0.4308   pool 0.3818
    windowed conv 0.0281      small GEMM fp32 0.0107
    stem VALU <4,8> 0.0021    <5,6> 0.0047    its per-peak sums 0.0003
    stem fused U = 18 0.0006  U = 40 0.0006   its per-peak sums 0.0002
The sums stay far below 1 because the bound counts every term at its worst sign (n_acc u Cabs) while rounding errors of a few
thousand terms add like a random walk; the pointwise ratios are what round-to-nearest operations give against k that counts the divide 3.
"""
import collections
import functools
import math
import zlib

import numpy as np
import torch

F32, F64 = np.float32, np.float64
EPS = np.float32(1e-10)            # peak_backprop_3d.py:30, as the fp32 run sees it
U24 = 2.0 ** -24
C3 = 2.0                           # tests/f16x2_contract.py
DIV = 3
LIMIT = 2.0 ** 24

NORM_EDGES = (0.0, 5e-11, float(EPS), float(np.nextafter(EPS, F32(0))), float(np.nextafter(EPS, F32(1))), -1.0, -1e3, 1e-9, 1e3)
XNEXT_EDGES = (0.0, -0.0, float(np.finfo(F32).tiny), -float(np.finfo(F32).tiny), -1.0, -3.5)


# ------------------------------------------------------------------ windows in virtual coordinates
def _overlap(origin, wshape, mshape):
    src, dst = [], []
    for o, w, m in zip(origin, wshape, mshape):
        o = int(o)
        lo, hi = max(0, o), min(m, o + w)
        if lo >= hi:
            return None, None
        src.append(slice(lo - o, hi - o))
        dst.append(slice(lo, hi))
    return tuple(src), tuple(dst)


def place(win, origin, shape):
    """win [C, a, b, c] whose voxel (0, 0, 0) sits at `origin` of a [C, *shape] map -> that map, zero outside the window"""
    out = np.zeros((win.shape[0],) + tuple(shape), win.dtype)
    src, dst = _overlap(origin, win.shape[1:], shape)
    if src is not None:
        out[(slice(None),) + dst] = win[(slice(None),) + src]
    return out


def crop(m, origin, n):
    """the [C, n, n, n] window of the map m [C, D, H, W] at `origin`, zero where it sticks out"""
    out = np.zeros((m.shape[0], n, n, n), m.dtype)
    src, dst = _overlap(origin, (n, n, n), m.shape[1:])
    if src is not None:
        out[(slice(None),) + src] = m[(slice(None),) + dst]
    return out


def inside_box(origin, n, shape):
    """slices of the part of an n^3 window at `origin` that lies inside a map of `shape`, or None"""
    return _overlap(origin, (n, n, n), shape)[0]


def unpool(g, argmax, shape):
    """max-unpool of MaxPool3d(2, 2): g [C, UD, UH, UW] goes to child argmax = 4 dz + 2 dy + dx of its 2x2x2 block of a [C, *shape] map"""
    Cc, UD, UH, UW = g.shape
    out = np.zeros((Cc,) + tuple(shape), g.dtype)
    c, z, y, x = np.meshgrid(np.arange(Cc), np.arange(UD), np.arange(UH), np.arange(UW), indexing="ij")
    a = argmax.astype(np.int64)
    qz, qy, qx = 2 * z + (a >> 2), 2 * y + ((a >> 1) & 1), 2 * x + (a & 1)
    ok = (qz < shape[0]) & (qy < shape[1]) & (qx < shape[2])
    out[c[ok], qz[ok], qy[ok], qx[ok]] = g[ok]
    return out


def pooled(m, argmax):
    """m [C, D, H, W] at the arg-max children: [C, UD, UH, UW] (0 where the child lies outside the map)"""
    Cc, UD, UH, UW = argmax.shape
    c, z, y, x = np.meshgrid(np.arange(Cc), np.arange(UD), np.arange(UH), np.arange(UW), indexing="ij")
    a = argmax.astype(np.int64)
    qz, qy, qx = 2 * z + (a >> 2), 2 * y + ((a >> 1) & 1), 2 * x + (a & 1)
    ok = (qz < m.shape[1]) & (qy < m.shape[2]) & (qx < m.shape[3])
    out = np.zeros(argmax.shape, m.dtype)
    out[ok] = m[c[ok], qz[ok], qy[ok], qx[ok]]
    return out, ok


def posthook(g, norm, dt=F64, abs_cut=False):
    """peak_backprop_3d.py:30-33.  abs_cut: the MUTANT that cuts at |norm| < eps"""
    cut = (np.abs(norm) < EPS) if abs_cut else (norm < EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = g / denominator(norm, dt)
    return np.where(cut, dt(0), q)


def denominator(norm, dt=F64):
    """|norm| + eps as the reference run computes it: ONE add in the norm's own format (fp32 for the kernels' inputs - a correctly
    rounded add is the same bits everywhere, and |n| + eps == |n| for the exact cases' powers of two), then exact in `dt`"""
    norm = np.asarray(norm)
    return (np.abs(norm) + norm.dtype.type(EPS)).astype(dt)


# ------------------------------------------------------------------ the stage references
def ref_seed(peaks, prob, ncls, wcls, h, h_off, dt=F64):
    """prm_seed_kernel: peaks [P,4] (a,s,h,w) -> ([P,C] = (h - off) relu(Wcls[a]) (1 - y) y / (|Ncls| + eps), origin (s,h,w))"""
    P, Cc = len(peaks), h.shape[0]
    out = np.zeros((P, Cc), dt)
    for p, (a, s, hh, w) in enumerate(np.asarray(peaks).tolist()):
        y = dt(prob[a, s, hh, w])
        g = (dt(1) - y) * y
        gn = posthook(np.asarray(g, dt), np.asarray(ncls[a, s, hh, w]), dt)
        out[p] = (h[:, s, hh, w].astype(dt) - dt(h_off)) * (np.maximum(wcls[a].astype(dt), dt(0)) * gn)
    return out, np.asarray(peaks)[:, 1:4].astype(np.int32)


def ref_prepare(gup, origin_up, pool, border, argmax, xnext, scale, norm, up_off=None, dt=F64, abs_cut=False):
    """m3d_prm_prepare_ex3 on batch-major windows: gup [P,C,U,U,U] at origin_up (coordinates of xnext [C,UD,UH,UW]) ->
    (G_N [P,C,Wn,Wn,Wn], origin_out), Wn = (2 if pool else 1) U + 2 border, origin_out = (2 if pool else 1) origin_up - border"""
    P, Cc, U = gup.shape[:3]
    mul = 2 if pool else 1
    Wn = mul * U + 2 * border
    origin_out = (mul * np.asarray(origin_up, np.int64) - border).astype(np.int32)
    out = np.zeros((P, Cc, Wn, Wn, Wn), dt)
    xn = xnext.astype(dt)
    for p in range(P):
        g = place(gup[p].astype(dt), origin_up[p], xnext.shape[1:])
        live = place(np.ones((Cc, U, U, U), bool), origin_up[p], xnext.shape[1:])
        if up_off is not None:
            g = (xn - dt(up_off)) * g                                   # PreHook of the layer above, peak_backprop_3d.py:16-18
        g = np.where(xnext > 0, g, dt(0))                               # ReLU backward
        if scale is not None:
            g = g * scale.astype(dt)[:, None, None, None]               # eval-mode BatchNorm backward
        if pool:
            g, live = unpool(g, argmax, norm.shape[1:]), unpool(live, argmax, norm.shape[1:])
        g = np.where(live, posthook(g, norm, dt, abs_cut), dt(0))
        out[p] = crop(g, origin_out[p], Wn)
    return out, origin_out


def k_prepare(up_off, scale):
    return 1 + DIV + (2 if up_off else 0) + (1 if scale else 0)


def ref_den_pool(argmax, xnext, norm, dt=F64):
    """m3d_prm_den_pool: |N| + eps at the arg-max child where the pooled activation is > 0 and not N < eps, else 0"""
    n, ok = pooled(norm, argmax)
    return np.where((xnext > 0) & ok & ~(n < EPS), denominator(n, dt), dt(0))


def _conv_input(g, w, k, dt):
    """backward-data of the 'same' conv with weight w [cg, cx, k, k, k]: g [B, cg, ...] -> [B, cx, ...]"""
    tt = torch.float64 if dt is F64 else torch.float32
    g, w = torch.from_numpy(np.ascontiguousarray(g)).to(tt), torch.from_numpy(np.ascontiguousarray(w)).to(tt)
    shape = (g.shape[0], w.shape[1]) + tuple(g.shape[2:])
    return torch.nn.grad.conv3d_input(shape, w, g, padding=k // 2).numpy()


def ref_dgrad(gn, w, full, off, origin, dt=F64, want_cabs=False):
    """windowed backward-data + PreHook: gn [P,cg,n,n,n], w [cg,cx,3,3,3] (the forward conv's weight), full [cx,D,H,W] ->
    conv_transpose(gn, relu(w)) * (full[origin + v] - off), 0 outside the map  (+ Cabs |full - off| for the bound)"""
    n = gn.shape[2]
    wp = np.maximum(w.astype(dt), dt(0))
    m = np.stack([crop(full.astype(dt) - dt(off), o, n) for o in origin])
    inmap = np.stack([crop(np.ones(full.shape, bool), o, n) for o in origin])
    y = np.where(inmap, m * _conv_input(gn.astype(dt), wp, 3, dt), dt(0))
    if not want_cabs:
        return y
    return y, np.where(inmap, np.abs(m) * _conv_input(np.abs(gn.astype(dt)), wp, 3, dt), dt(0))


def _stem_conv(gn, w, dt, box=None):
    """sum_{c,t} relu(W)[c][124 - t] gn[c][v + t - 2] for gn [C,n,n,n]; box: only there (gn must vanish outside it)"""
    wp = np.maximum(w.astype(dt), dt(0))
    if box is None:
        return _conv_input(gn[None], wp, 5, dt)[0, 0]
    out = np.zeros(gn.shape[1:], dt)
    assert np.count_nonzero(gn) == np.count_nonzero(gn[(slice(None),) + box]), "G_N outside the map"
    out[box] = _conv_input(gn[(slice(None),) + box][None], wp, 5, dt)[0, 0]
    return out


def ref_stem(gn, w, data, off, origin, dt=F64, want_cabs=False, boxed=False):
    """m3d_prm_stem_dgrad: gn [P,C,n,n,n], w [C,1,5,5,5] -> (clamp((data - off) conv, 0) [P,n,n,n], per-peak sums [, bound term])"""
    P, n = gn.shape[0], gn.shape[2]
    y, ca = np.zeros((P, n, n, n), dt), np.zeros((P, n, n, n), dt)
    for p in range(P):
        box = inside_box(origin[p], n, data.shape)
        if box is None:
            continue
        m = crop((data.astype(dt) - dt(off))[None], origin[p], n)[0]
        g = gn[p].astype(dt)
        y[p] = np.maximum(m * _stem_conv(g, w, dt, box if boxed else None), dt(0))
        if want_cabs:
            ca[p] = np.abs(m) * _stem_conv(np.abs(g), w, dt, box if boxed else None)
    inmap = np.stack([crop(np.ones((1,) + data.shape, bool), o, n)[0] for o in origin])
    y = np.where(inmap, y, dt(0))
    sums = y.reshape(P, -1).sum(1)
    return (y, sums, np.where(inmap, ca, dt(0))) if want_cabs else (y, sums)


def ref_fused_gn(gup, origin_up, den, argmax, scale, shape, xnext=None, up_off=None, dt=F64):
    """the G_N windows the fused stem kernel stages: gup [P,32,U,U,U] -> ([P,32,Wn,Wn,Wn], origin 2 origin_up - 2), Wn = 2 U + 4"""
    P, Cc, U = gup.shape[:3]
    Wn = 2 * U + 4
    origin_out = (2 * np.asarray(origin_up, np.int64) - 2).astype(np.int32)
    out = np.zeros((P, Cc, Wn, Wn, Wn), dt)
    for p in range(P):
        g = place(gup[p].astype(dt), origin_up[p], den.shape[1:])
        if up_off is not None:
            g = (xnext.astype(dt) - dt(up_off)) * g
        if scale is not None:
            g = g * scale.astype(dt)[:, None, None, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.where(den > 0, g / den.astype(dt), dt(0))
        out[p] = crop(unpool(g, argmax, shape), origin_out[p], Wn)
    return out, origin_out


def ref_stem_fused(gup, origin_up, den, argmax, scale, w, data, off, xnext=None, up_off=None, dt=F64, want_cabs=False):
    """m3d_prm_stem_dgrad_fused_ex2 -> (windows [P,Wn,Wn,Wn], sums, origins [, bound term]); only the part of a window inside the
    volume is convolved (G_N vanishes outside it, asserted)"""
    parts, origin = [], []
    for p in range(gup.shape[0]):                                       # peak by peak: a 84^3 x 32 fp64 window is 150 MB
        gn, o = ref_fused_gn(gup[p:p + 1], origin_up[p:p + 1], den, argmax, scale, data.shape, xnext, up_off, dt)
        parts.append(ref_stem(gn, w, data, off, o, dt, want_cabs, boxed=True))
        origin.append(o)
    return (np.concatenate([r[0] for r in parts]), np.concatenate([r[1] for r in parts]), np.concatenate(origin)) + \
        ((np.concatenate([r[2] for r in parts]),) if want_cabs else ())


def k_fused(up_off, scale):
    return 1 + DIV + (2 if up_off else 0) + (1 if scale else 0)


def ref_scatter(win, sums, origin, shape, dt=F64):
    """m3d_prm_scatter: dense [P,D,H,W] = window / sum at the origin, 0 / sum elsewhere (a zero sum: NaN everywhere)"""
    P, n = win.shape[:2]
    out = np.zeros((P,) + tuple(shape), dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        for p in range(P):
            s = dt(sums[p])
            out[p] = dt(0) / s
            src, dst = _overlap(origin[p], (n, n, n), shape)
            if src is not None:
                out[p][dst] = win[p][src].astype(dt) / s
    return out


def sum_adds(w3):
    """adds a value passes on its way through window_sums_kernel (1024 threads; csrc/prm.hip)"""
    return (2 + math.ceil(w3 / 4096) + 10) if w3 % 4 == 0 else (math.ceil(w3 / 1024) + 10)


# ------------------------------------------------------------------ bounds and comparisons
def bound_pointwise(y, k):
    return k * U24 * np.abs(y)


def bound_sum(y, cabs, terms, k_g=0, clamped=False):
    """cabs = Cabs |X - off|.  clamped (the stems' clamp(min = 0)): |max(a, 0) - max(b, 0)| <= |a - b|, and the un-clamped |y| that the
    last two roundings scale with is at most cabs"""
    return (C3 * (terms + 3) + k_g) * U24 * cabs + 2 * U24 * (cabs if clamped else np.abs(y))


def ratio_sums(got_sums, got_win, y, bound, w3, what):
    """worst |got - sum y| / bound of the per-peak sums (the module docstring's bound)"""
    P = y.shape[0]
    want = y.reshape(P, -1).sum(1)
    b = bound.reshape(P, -1).sum(1) + sum_adds(w3) * U24 * np.abs(np.asarray(got_win, F64)).reshape(P, -1).sum(1)
    err = np.abs(np.asarray(got_sums, F64) - want)
    assert np.all(err[b == 0] == 0), what + ": a sum differs where nothing may"
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def same_bits(got, ref, what, sums=False):
    """bit-equal to the fp64 reference cast to fp32 (NaN == NaN); sums: the sign of a zero is not compared"""
    got, ref = np.asarray(got, F32), np.asarray(ref).astype(F32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if sums:
        got, ref = got + F32(0), ref + F32(0)
    bad = got.view(np.uint32) != ref.view(np.uint32)
    bad &= ~(np.isnan(got) & np.isnan(ref))
    if bad.any():
        idx = np.argwhere(bad)
        raise AssertionError("%s: %d of %d elements differ; first %s got %r want %r; last %s"
                             % (what, len(idx), ref.size, idx[0].tolist(), float(got[tuple(idx[0])]), float(ref[tuple(idx[0])]),
                                idx[-1].tolist()))


def ratio(got, y, bound, what, signs=True):
    """worst |got - y| / bound over all elements, none of which may err where the bound is zero (outside the map, gaps of a strip);
    signs (the pointwise stages): zeros of y must be exact zeros of got and the signs agree"""
    got = np.asarray(got).astype(F64)
    assert got.shape == y.shape, (what, got.shape, y.shape)
    nan = np.isnan(y)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN pattern"
    g, yy, b = got[~nan], y[~nan], bound[~nan]
    assert np.all(np.isfinite(g)), what + ": not finite"
    if signs:
        zero = yy == 0
        assert not np.any(g[zero]), what + ": %d non-zero where the reference is exactly zero" % int(np.count_nonzero(g[zero]))
        assert np.array_equal(np.sign(g[~zero]), np.sign(yy[~zero])), what + ": sign"
    err = np.abs(g - yy)
    live = err > 0
    if not live.any():
        return 0.0
    assert np.all(b[live] > 0), what + ": an error where the bound is zero"
    return float((err[live] / b[live]).max())


# ------------------------------------------------------------------ strip layouts (include/m3d.h: m3d_prm_strip_geometry)
def strip_geometry(n, mode, P):
    """(pitch, lead, L): mode 1: pitch n + 1, lead 0, L = P (n + 1); mode 2: the start residue r = lead in 0..3 (first wins) with the
    smallest pitch = the smallest multiple of 4 > max(n + r, 4 floor((r + n - 1) / 4) + 4 - r), L = P pitch + roundup(lead, 4)"""
    if mode == 1:
        return n + 1, 0, P * (n + 1)
    assert mode == 2
    best = None
    for r in range(4):
        m = max(n + r, 4 * ((r + n - 1) // 4) + 4 - r)
        pitch = 4 * (m // 4 + 1)
        if best is None or pitch < best[0]:
            best = (pitch, r)
    return best[0], best[1], P * best[0] + (4 if best[1] else 0)


def pack_strip(win, mode, origin_z=None, zn=None, fill=0.0):
    """batch-major [P,C,n,n,n] -> strip [C,n,n,L] (mode 1 / 2; mode 0 returns win); with (origin_z [P], zn) the slab strip [C,zn,n,L]
    whose plane k holds plane k - origin_z[p] of window p.  Lead, separators, tail and the slab planes no window covers are `fill`."""
    if not mode:
        return win
    P, Cc, n = win.shape[:3]
    pitch, lead, L = strip_geometry(n, mode, P)
    out = np.full((Cc, n if zn is None else zn, n, L), fill, win.dtype)
    for p in range(P):
        cols = slice(lead + p * pitch, lead + p * pitch + n)
        if zn is None:
            out[:, :, :, cols] = win[p]
        else:
            out[:, :, :, cols] = crop_z(win[p], -int(origin_z[p]), zn, fill)
    return out


def crop_z(w, start, zn, fill=0.0):
    """planes start .. start + zn - 1 of w [C,n,a,b] (`fill` where there is none)"""
    out = np.full((w.shape[0], zn) + w.shape[2:], fill, w.dtype)
    lo, hi = max(0, start), min(w.shape[1], start + zn)
    if lo < hi:
        out[:, lo - start:hi - start] = w[:, lo:hi]
    return out


def unpack_strip(strip, mode, P, n, origin_z=None):
    """the windows [P,C,n,n,n] of a strip (slab: with origin_z; planes outside the slab come back as zero)"""
    if not mode:
        return strip
    pitch, lead, L = strip_geometry(n, mode, P)
    assert strip.shape[-1] == L and strip.shape[2] == n
    out = np.zeros((P, strip.shape[0], n, n, n), strip.dtype)
    for p in range(P):
        w = strip[:, :, :, lead + p * pitch:lead + p * pitch + n]
        out[p] = w if origin_z is None else crop_z(w, int(origin_z[p]), n)
    return out


def gap_columns(mode, P, n):
    """the columns of a strip row that belong to no window: lead, separators, tail"""
    pitch, lead, L = strip_geometry(n, mode, P)
    own = np.zeros(L, bool)
    for p in range(P):
        own[lead + p * pitch:lead + p * pitch + n] = True
    return np.nonzero(~own)[0]


# ------------------------------------------------------------------ case tables
PREPARE_KERNELS = ("element", "quad<8>", "quad<16>", "quad<32>", "pool")
STEM_LAYOUTS = ("<4,8>", "<5,6>")

# shape = this layer's map (D, H, W); pool cases: xnext is (D // 2, H // 2, W // 2) - odd extents, so MaxPool3d's floor applies.
# origins: "edge" = a negative origin, an interior one and one at the far corner; "out" = the interior one replaced by a window that lies
# wholly outside the map.  in_l / out_l: 0 batch-major, 1 strip (pitch n + 1), 2 quad-aligned strip.
PrepCase = collections.namedtuple("PrepCase", "kernel C U pool border shape in_l out_l in_slab out_slab up_off scale origins")


def _prep_cases():
    out = []
    k = 0

    def add(kernel, Cc, U, pool, border, shapes, outs, ins=(0, 1, 2)):
        nonlocal k
        for out_l in outs:
            for in_l in ins:
                shape = shapes[k % len(shapes)]
                up = tuple(s // 2 for s in shape) if pool else shape
                Wn = (2 if pool else 1) * U + 2 * border
                # slab strips where the map is thinner than the window, in every second case that admits one; up_off / scale / origins rotate
                in_slab = bool(in_l) and up[0] < U and k % 5 < 3
                out_slab = bool(out_l) and shape[0] < Wn and k % 2 == 0
                out.append(PrepCase(kernel, Cc, U, pool, border, shape, in_l, out_l, in_slab, out_slab, k % 4 in (1, 2),
                                    (True, False, True, True, False)[k % 5], ("edge", "out")[(k // 3) % 2]))
                k += 1

    small = ((5, 6, 7), (7, 9, 6), (12, 14, 16))
    for U in (1, 3, 5):
        for border in (1, 2):
            add("element", 3, U, False, border, ((5, 6, 7), (4, 9, 6), (12, 14, 16)), (0, 1))
    add("quad<8>", 3, 3, False, 1, small, (2,))                      # Wn 5: pitch 8
    add("quad<8>", 3, 14, False, 1, small, (2,))                     # Wn 16: pitch 20, lead 0
    add("quad<8>", 3, 14, False, 2, small, (2,))                     # Wn 18: pitch 20, lead 1
    add("quad<16>", 3, 36, False, 1, small, (2,))                    # Wn 38: pitch 40, lead 1
    add("quad<16>", 3, 36, False, 2, small, (2,))                    # Wn 40: pitch 44, lead 0
    add("quad<32>", 2, 60, False, 1, small, (2,))                    # Wn 62: pitch 64, lead 1 (17 quads with the tail)
    add("quad<32>", 1, 62, False, 1, small, (2,), ins=(0,))          # Wn 64: pitch 68
    odd = ((7, 9, 11), (11, 13, 15), (9, 7, 13))
    for U in (3, 7):
        for border in (1, 2):
            add("pool", 3, U, True, border, odd, (0, 1, 2))
    return tuple(out)


PREP_CASES = _prep_cases()


def prep_id(c):
    return "%s-c%d-u%d-b%d-%dx%dx%d-in%d%s-out%d%s%s%s-%s" % (c.kernel.replace("<", "").replace(">", ""), c.C, c.U, c.border, c.shape[0], c.shape[1],
                                                              c.shape[2], c.in_l, "s" if c.in_slab else "", c.out_l, "s" if c.out_slab else "",
                                                              "-off" if c.up_off else "", "-bn" if c.scale else "", c.origins)


def origins_for(kind, up_shape, U, P=3):
    """P = 3 window origins in the coordinates of a map of up_shape for windows U wide"""
    UD, UH, UW = up_shape
    neg = (-(U // 2) - 1, -1, -(U // 2)) if U > 2 else (0, 0, 0)      # (a 1^3 window: its OUTPUT window still starts at -border)
    mid = (min(1, UD - 1), min(2, UH - 1), 1)
    far = (UD - 1, UH - 2, UW - 1)
    outside = (UD + 3, 0, -U - 2)                                     # beyond the map in z and in x
    return np.array([neg, outside if kind == "out" else mid, far][:P], np.int32)


def _seed_of(case, salt):
    return zlib.crc32(repr(tuple(case)).encode()) + salt


def sprinkle(a, values, rng, frac=0.3):
    """a with a fraction of its elements replaced by the given edge values"""
    a = a.copy()
    m = rng.random(a.shape) < frac
    a[m] = rng.choice(np.asarray(values, F32), size=int(m.sum()))
    return a


def exact_norm(shape, rng):
    """norms whose PostHook is exact: 0, below eps, negative (all -> 0) and powers of two >= 2^-9 (|n| + eps == |n| in fp32)"""
    n = (2.0 ** rng.integers(-9, 4, shape)).astype(F32)
    assert np.array_equal(n + EPS, n)
    return sprinkle(n, (0.0, 5e-11, float(np.nextafter(EPS, F32(0))), -1.0, -4.0), rng, 0.25)


def random_norm(shape, rng):
    n = (10.0 ** rng.uniform(-9, 3, shape)).astype(F32)
    return sprinkle(n, NORM_EDGES, rng, 0.25)


def prep_inputs(c, exact):
    """every operand of one prepare case as fp32 numpy arrays (batch-major gup; the GPU test packs it)"""
    rng = np.random.default_rng(_seed_of(c, 1 if exact else 2))
    P = 3
    up = tuple(s // 2 for s in c.shape) if c.pool else c.shape
    gshape = (P, c.C, c.U, c.U, c.U)
    if exact:
        gup = rng.integers(-3, 4, gshape).astype(F32)
        up_off = F32(-2.0)
        xnext = sprinkle(rng.integers(-2, 4, (c.C,) + up).astype(F32), XNEXT_EDGES[:4], rng, 0.15)
        scale = np.array([-2.0, 1.0, 3.0, -1.0][:c.C], F32)
        norm = exact_norm((c.C,) + c.shape, rng)
    else:
        gup = (rng.standard_normal(gshape) * 10.0 ** rng.uniform(-3, 3, (P, 1, 1, 1, 1))).astype(F32)
        xnext = sprinkle(rng.standard_normal((c.C,) + up).astype(F32) + F32(0.5), XNEXT_EDGES, rng, 0.15)
        up_off = xnext.min()
        scale = (rng.uniform(0.5, 1.5, c.C) * np.array([-1, 1, 1, -1][:c.C])).astype(F32)
        norm = random_norm((c.C,) + c.shape, rng)
    argmax = rng.integers(0, 8, (c.C,) + up).astype(np.uint8) if c.pool else None
    origin_up = origins_for(c.origins, up, c.U, P)
    # the first and the last peak reach the map with few voxels: keep one of them alive, so that neither window is all zero
    for p, v in ((0, tuple(max(0, int(o)) for o in origin_up[0])), (2, tuple(min(s - 1, int(o) + c.U - 1) for s, o in zip(up, origin_up[2])))):
        xnext[(slice(None),) + v] = 2
        q = v
        if c.pool:
            argmax[(slice(None),) + v] = 5
            q = (2 * v[0] + 1, 2 * v[1], 2 * v[2] + 1)
        norm[(slice(None),) + q] = 0.5
        gup[(p, slice(None)) + tuple(int(a - o) for a, o in zip(v, origin_up[p]))] = 3
    if not exact:
        up_off = xnext.min()
    return dict(gup=gup, origin_up=origin_up, argmax=argmax, xnext=xnext, scale=scale if c.scale else None,
                norm=norm, up_off=up_off if c.up_off else None)


def prep_reference(c, inp, **kw):
    return ref_prepare(inp["gup"], inp["origin_up"], c.pool, c.border, inp["argmax"], inp["xnext"], inp["scale"], inp["norm"],
                       inp["up_off"], **kw)


def prep_layouts(c, inp, ref, origin_out, fill=0.0):
    """(gup as the case's input layout, the reference as its output layout - every column: lead, separators, tail, slab planes)"""
    gin = pack_strip(inp["gup"], c.in_l, inp["origin_up"][:, 0] if c.in_slab else None, inp["xnext"].shape[1] if c.in_slab else None)
    want = pack_strip(ref, c.out_l, origin_out[:, 0] if c.out_slab else None, c.shape[0] if c.out_slab else None, fill)
    return gin, want


# ---- seed / den_pool / scatter
SeedCase = collections.namedtuple("SeedCase", "A C shape P")
SEED_CASES = (SeedCase(3, 5, (5, 6, 7), 3), SeedCase(35, 70, (2, 3, 5), 37), SeedCase(2, 257, (1, 1, 3), 5))


def seed_inputs(c, exact):
    rng = np.random.default_rng(_seed_of(c, 11 if exact else 12))
    S, H, W = c.shape
    peaks = np.stack([rng.integers(0, c.A, c.P), rng.integers(0, S, c.P), rng.integers(0, H, c.P), rng.integers(0, W, c.P)], 1).astype(np.int32)
    peaks[0, 1:] = (S - 1, H - 1, W - 1)
    peaks[-1, 1:] = 0
    if exact:
        # y = 1/2, 1/4 or 3/4: (1 - y) y = 1/4 or 3/16, exact; everything else integer
        prob = rng.choice(np.array([0.5, 0.25, 0.5, 0.75, 1.0, 0.0], F32), (c.A,) + c.shape)
        ncls = exact_norm((c.A,) + c.shape, rng)
        prob[tuple(peaks[0])], ncls[tuple(peaks[0])] = 0.25, 0.5             # one peak that is certainly alive
        wcls = rng.integers(-3, 4, (c.A, c.C)).astype(F32)
        h = rng.integers(0, 6, (c.C,) + c.shape).astype(F32)
        off = F32(-1.0)
    else:
        prob = (1.0 / (1.0 + np.exp(-rng.standard_normal((c.A,) + c.shape) * 6))).astype(F32)
        ncls = random_norm((c.A,) + c.shape, rng)
        wcls = rng.standard_normal((c.A, c.C)).astype(F32)
        h = np.maximum(rng.standard_normal((c.C,) + c.shape), 0).astype(F32) * F32(10.0 ** rng.uniform(-2, 2))
        off = h.min()
    return dict(peaks=peaks, prob=prob, ncls=ncls, wcls=wcls, h=h, off=off)


DEN_CASES = ((3, (7, 9, 11)), (32, (5, 4, 7)), (1, (2, 2, 2)), (2, (6, 8, 10)))          # (C, this layer's map)


def den_inputs(case, exact):
    Cc, shape = case
    rng = np.random.default_rng(_seed_of(case, 21 if exact else 22))
    up = tuple(s // 2 for s in shape)
    argmax = rng.integers(0, 8, (Cc,) + up).astype(np.uint8)
    xnext = sprinkle(rng.standard_normal((Cc,) + up).astype(F32), XNEXT_EDGES, rng, 0.3)
    norm = exact_norm((Cc,) + shape, rng) if exact else random_norm((Cc,) + shape, rng)
    return dict(argmax=argmax, xnext=xnext, norm=norm)


ScatterCase = collections.namedtuple("ScatterCase", "win shape")
SCATTER_CASES = (ScatterCase(5, (5, 6, 7)),        # 210 voxels: not a multiple of 4 (dword fill)
                 ScatterCase(20, (12, 14, 16)),    # float4 fill, windows larger than the map
                 ScatterCase(3, (3, 3, 3)))        # 27 voxels


def scatter_inputs(c, exact):
    """P = 4: negative, interior / outside, far corner, and a peak whose sum is zero (its map: NaN everywhere)"""
    rng = np.random.default_rng(_seed_of(c, 31 if exact else 32))
    P = 4
    origin = np.concatenate([origins_for("out" if c.win == 5 else "edge", c.shape, c.win), [[0, 1, -1]]]).astype(np.int32)
    if exact:
        win = rng.integers(0, 9, (P, c.win, c.win, c.win)).astype(F32)
        sums = np.array([4.0, 0.5, 16.0, 0.0], F32)
    else:
        win = np.abs(rng.standard_normal((P, c.win, c.win, c.win)) * 10.0 ** rng.uniform(-3, 3, (P, 1, 1, 1))).astype(F32)
        sums = win.reshape(P, -1).sum(1).astype(F32)
        sums[3] = 0
    win[3] = 0
    return dict(win=win, sums=sums, origin=origin)


# ---- windowed direct conv (W_DGRAD_RELU pack + PreHook epilogue) and the small-window GEMM (fp32)
# cg = channels of G_N (the forward conv's cout: odd), cx = channels of X (the forward conv's cin: ragged against the 32-channel blocks)
DgradCase = collections.namedtuple("DgradCase", "win cg cx shape P variant")
WINDOWED_CASES = (
    DgradCase(3, 3, 20, (5, 6, 7), 3, 2), DgradCase(7, 5, 40, (5, 6, 7), 3, 12), DgradCase(9, 7, 20, (7, 9, 6), 3, 1),
    DgradCase(9, 3, 70, (12, 14, 16), 3, 9), DgradCase(18, 5, 40, (12, 14, 16), 3, 12), DgradCase(18, 3, 20, (5, 6, 7), 3, 2),
    DgradCase(18, 17, 70, (12, 14, 16), 3, 12),
)
SMALL_CASES = tuple(DgradCase(win, 7, 40, (5, 6, 7), P, None) for win in (3, 5, 7) for P in (1, 37))


def dgrad_id(c):
    return "w%d-%dto%d-%dx%dx%d-p%d" % ((c.win, c.cg, c.cx) + c.shape + (c.P,))


def dgrad_inputs(c, exact):
    rng = np.random.default_rng(_seed_of(c, 41 if exact else 42))
    D, H, W = c.shape
    if c.P == 3:
        origin = origins_for("out" if c.win == 7 else "edge", c.shape, c.win)
    else:
        origin = np.stack([rng.integers(-c.win - 1, D + 2, c.P), rng.integers(-c.win - 1, H + 2, c.P), rng.integers(-c.win - 1, W + 2, c.P)], 1).astype(np.int32)
        origin[0] = (0, 0, 0) if c.P == 1 else (-1, -2, -1)
    gshape = (c.P, c.cg) + (c.win,) * 3
    if exact:
        gn = rng.integers(-3, 4, gshape).astype(F32)
        w = rng.integers(-2, 3, (c.cg, c.cx, 3, 3, 3)).astype(F32)
        full = rng.integers(-1, 5, (c.cx,) + c.shape).astype(F32)
        off = F32(1.0)                                                  # X - off in -2 .. 3: the PreHook factor has both signs
    else:
        gn = (rng.standard_normal(gshape) * 10.0 ** rng.uniform(-3, 3, (c.P, 1, 1, 1, 1))).astype(F32)
        w = (rng.standard_normal((c.cg, c.cx, 3, 3, 3)) * (2.0 / (27 * c.cg)) ** 0.5).astype(F32)
        full = rng.standard_normal((c.cx,) + c.shape).astype(F32)
        off = full.min()
    return dict(gn=gn, w=w, full=full, off=off, origin=origin)


# ---- stem: VALU form (one case per thread layout and channel count, + an odd window for the dword path of the per-peak sums) and the
# fused MFMA form (its two instantiations, U = 18 and 40; 32 channels)
StemCase = collections.namedtuple("StemCase", "win C shape layout")
STEM_CASES = (StemCase(40, 3, (12, 14, 16), "<5,6>"), StemCase(20, 32, (12, 14, 16), "<4,8>"), StemCase(20, 3, (7, 9, 6), "<4,8>"),
              StemCase(40, 32, (9, 45, 50), "<5,6>"), StemCase(9, 3, (5, 6, 7), "<4,8>"))


def stem_inputs(c, exact):
    rng = np.random.default_rng(_seed_of(c, 51 if exact else 52))
    P = 3
    origin = origins_for("out" if c.win == 20 and c.C == 3 else "edge", c.shape, c.win)
    gshape = (P, c.C) + (c.win,) * 3
    if exact:
        gn = rng.integers(-3, 4, gshape).astype(F32)
        w = rng.integers(-2, 3, (c.C, 1, 5, 5, 5)).astype(F32)
        data = rng.integers(0, 4, c.shape).astype(F32)
        off = F32(1.0)                                                  # data - off in -1 .. 2: the clamp matters
    else:
        gn = (rng.standard_normal(gshape) * 10.0 ** rng.uniform(-3, 3, (P, 1, 1, 1, 1))).astype(F32)
        w = (rng.standard_normal((c.C, 1, 5, 5, 5)) * (2.0 / 125) ** 0.5).astype(F32)
        data = rng.standard_normal(c.shape).astype(F32)
        off = data.min()
    return dict(gn=gn, w=w, data=data, off=off, origin=origin)


# pooled = the pooled stem map (UD, UH, UW); data is 2 pooled (+ 1 where odd: MaxPool3d floors).  in_l: layout of gup; slab with strips.
FusedCase = collections.namedtuple("FusedCase", "U pooled odd P in_l slab up_off scale")
def _fused_cases():
    """U = 18: every layout of gup (batch-major, strip 1, strip 2, and the two as slab strips) with and without (xnext, up_off);
    U = 40: every layout once, the PreHook alternating, on thin maps (one of them wide enough to hold whole rows of a window)"""
    layouts = ((0, False), (1, False), (2, False), (1, True), (2, True))
    maps18 = ((6, 7, 8), (5, 21, 9), (6, 7, 8), (4, 9, 23), (6, 7, 8))
    out = []
    for i, (in_l, slab) in enumerate(layouts):
        for up_off in (False, True):
            out.append(FusedCase(18, maps18[i], (i + up_off) % 2 == 0, 3, in_l, slab, up_off, None if (i + up_off) % 3 == 1 else True))
    maps40 = ((6, 20, 45), (6, 8, 9), (6, 8, 9), (5, 9, 8), (6, 8, 9))
    for i, (in_l, slab) in enumerate(layouts):
        out.append(FusedCase(40, maps40[i], i % 2 == 0, 2, in_l, slab, i % 2 == 1, None if i == 2 else True))
    out.append(FusedCase(40, (6, 8, 9), False, 2, 0, False, True, True))
    return tuple(out)


FUSED_CASES = _fused_cases()


def fused_id(c):
    return "u%d-%dx%dx%d%s-in%d%s%s%s" % ((c.U,) + c.pooled + ("-odd" if c.odd else "", c.in_l, "s" if c.slab else "", "-off" if c.up_off else "",
                                                            "-bn" if c.scale else ""))


def fused_inputs(c, exact):
    rng = np.random.default_rng(_seed_of(c, 61 if exact else 62))
    Cc = 32
    shape = tuple(2 * s + (1 if c.odd else 0) for s in c.pooled)
    origin_up = origins_for("edge", c.pooled, c.U, 3)[[0, 2] if c.P == 2 else [0, 1, 2]]
    gshape = (c.P, Cc) + (c.U,) * 3
    argmax = rng.integers(0, 8, (Cc,) + c.pooled).astype(np.uint8)
    if exact:
        gup = rng.integers(-3, 4, gshape).astype(F32)
        den = rng.integers(0, 2, (Cc,) + c.pooled).astype(F32)
        scale = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], F32), Cc)
        xnext = rng.integers(-1, 4, (Cc,) + c.pooled).astype(F32)
        up_off = F32(-1.0)
        w = rng.integers(-2, 3, (Cc, 1, 5, 5, 5)).astype(F32)
        data = rng.integers(0, 4, shape).astype(F32)
        off = F32(1.0)
    else:
        gup = (rng.standard_normal(gshape) * 10.0 ** rng.uniform(-3, 3, (c.P, 1, 1, 1, 1))).astype(F32)
        den = sprinkle((10.0 ** rng.uniform(-3, 3, (Cc,) + c.pooled)).astype(F32), (0.0,), rng, 0.3)
        scale = (rng.uniform(0.5, 1.5, Cc) * rng.choice([-1.0, 1.0], Cc)).astype(F32)
        xnext = np.maximum(rng.standard_normal((Cc,) + c.pooled), 0).astype(F32)
        up_off = xnext.min()
        w = (rng.standard_normal((Cc, 1, 5, 5, 5)) * (2.0 / 125) ** 0.5).astype(F32)
        data = rng.standard_normal(shape).astype(F32)
        off = data.min()
    return dict(gup=gup, origin_up=origin_up, den=den, argmax=argmax, scale=scale if c.scale else None, w=w, data=data, off=off,
                xnext=xnext if c.up_off else None, up_off=up_off if c.up_off else None)


@functools.lru_cache(maxsize=None)
def fused_reference(c, exact):
    """(inputs, windows, sums, origins, bound term) of a fused-stem case, computed once per process"""
    inp = fused_inputs(c, exact)
    y, s, o, ca = ref_stem_fused(inp["gup"], inp["origin_up"], inp["den"], inp["argmax"], inp["scale"], inp["w"], inp["data"], inp["off"],
                                 inp["xnext"], inp["up_off"], want_cabs=True)
    return inp, y, s, o, ca
