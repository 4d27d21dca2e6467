"""The per-element accuracy contract of the "f16x2" kernels, with fp64 references and a CPU emulation of the cut (no GPU needed).

The cut.  An fp32 operand `a` of a group whose magnitudes are bounded by A is multiplied by the power of two s = f16_scale_of(A)
(csrc/m3d_common.h: A s in [2^14, 2^15)), v = a s (exact), and cut into h = fp16(v), l = fp16(v - h) (round to nearest even, fp16
subnormals kept; v - h is exact in fp32).  The kernel multiplies the pieces of a and b in three fp16 MFMA products, h_a h_b + h_a l_b +
l_a h_b (each exact in fp32), accumulates in fp32 and multiplies the sum by 1 / (s_a s_b) (exact).

Error of one operand (unscaled units):  h normal: |v - h| <= 2^-11 |v|; v - h is cut again: |v - h - l| <= 2^-11 |v - h| + 2^-25
(the last for an fp16-subnormal l, half its 2^-24 spacing); h subnormal: |v - h| <= 2^-25 and l is 0 or 2^-24 with |v - h - l| <= 2^-25.
So e_a = |a - (h + l) / s| <= 2^-22 |a| + 2^-25 / s <= 2^-22 |a| + 2^-39 A   (1 / s <= A 2^-14), and |l / s| <= 2^-11 |a| + 2^-39 A.

Error of one product (dropped l_a l_b included):
  |a b - (h_a h_b + h_a l_b + l_a h_b) / (s_a s_b)| <= |a| e_b + |b| e_a + e_a e_b + |l_a l_b| / (s_a s_b)
     <= (3 2^-22 + 2^-44) |a b| + (1 + 2^-11 + 2^-22) 2^-39 (A |b| + B |a|) + 2^-77 A B.
A term with a = 0 or b = 0 is exact (the cut of 0 is 0).  Summed over the K terms of one output y = sum_k a_k b_k:

  |y^ - y| <= c1 2^-22 C + c2 2^-39 (A sum|b| + B sum|a|) + 2^-77 n A B + c3 n_acc 2^-24 (C + F) + 2^-24 |y|,   C = sum |a_k b_k|

with F the second term, sums over the terms whose a and b are both non-zero (n of them), c2 = 1.001 (1 + 2^-11 + 2^-22 rounded up) and:
  * c1 = 3 + 2^-22 from the cut, plus 2^-24 / 2^-22 = 0.25 for every operand the kernel itself rounds to fp32 before the cut;
  * c3 = 2: the f16 MFMA truncates when it adds into its fp32 accumulator (conv3d_zw.hip), an error below 2^-23 = 2 2^-24 of the
    running sum, whose magnitude is at most C + F; one such step per MFMA instruction (the 16 exact products of its K = 16 slice
    enter the accumulator together), plus one step for every further fp32 add or multiply on the accumulated value before the
    epilogue's last operation (split-K partial sums, the Winograd-z combination, scale multiplies);
  * 2^-24 |y|: the rounding of the output itself (the last fp32 operation: the shift / bias add or the final multiply).
The constants of the kernels (derived from their code, not fitted):

  kernel (call site)                        a (bound A)                  b (bound B)            c1     n_acc
  conv3d_zw.hip (ZwConv3d, + pool, strip)   V_k = d_a -+ d_b, fp32       U_k (fp64 -> fp32)     3.51   27 cin / 16 + 3
                                            (A = 2 in_max, per window)   (B = fl(1.5 max|w|))          (9 cin / 16 taps x chunks x 3
                                                                                                       MFMAs per M_k; + M0 + M1 + M2
                                                                                                       (2 adds) + scale multiply)
  fc_gemm.hip F16 (SplitLinearF16)          x (A = x_bound or max|x|)    W (B = max|W|)         3.01   3 K / 16 + 64
                                                                                                       (+ <= 64 split-K slices)
  conv3d_x3.hip x3f (X3Conv3d(f16=True))    fl(x - off)                  W or relu(W)           3.26   81 cin / 16 + cin / 32 + 1
                                            (A = fl(in_max - off))       (B = its max|.|)              (+ the K split's partials)
  prm_small_f16.hip (SmallWindowDgrad)      G_N of peak p                relu(W)                3.01   81 cout_fwd / 16 + cout_fwd / 32 + 2
                                            (A = max|G_N[p]|, per peak)  (B = max relu(W))             (+ tot += acc every 2 chunks;
                                                                                                       x (X - off) rounds once more)
                                            (f16_scale_of clamps s at 2^125: for A < 2^-111 the row holds with A_eff = max(A, 2^-111),
                                            for which 1 / s = 2^-125 <= A_eff 2^-14 - tests/prm_small_cases.py, clamp edge)
  roi_align3d.hip roi_align3d_fwd_gemm_kernel  f, the feature map       M[k][bin] = Wz Wy Wx   6.51   3 K / 16, K <= 128 voxels
    (roi_align3d_forward(feat_absmax=))     (A = feat_absmax)            (scale 2^14: B = 1)           (the un-scaling is exact)
The fc row assumes the planner's split-K (at most 64 slices); an OPT_TUNE_FC_SLICES override above 64 adds one step per slice.  The RoI
operator M is built in fp32 from the per-sample axis weights (roi_align_ref: the same fp32 sample positions): each axis weight carries
one rounding of 1 - l, at most three fp32 adds fold the samples and clamped duplicates of a bin onto one voxel (all terms >= 0, so the
error stays relative), and m = (wz wy) wx rounds twice: 3 (1 + 3) + 2 = 14 roundings of 2^-24 |m|, 3.5 2^-22 C, on top of the cut's 3.01.
The fused max pool and the ReLU are 1-Lipschitz: the pooled bound is the window's largest E.  A multiplier g after the sum (BN scale,
the PreHook's X - off) multiplies the whole bound.  Where C == 0 every term is exact: the output is exactly the shift / bias (or 0).
"""
import torch

F64 = torch.float64
C2 = 1.001
C3 = 2.0
KERNELS = {        # name: (c1, n_acc(k)) with k = cin (zw, x3f), K (fc), cout_fwd (prm_small)
    "zw": (3.51, lambda cin: 27 * cin / 16 + 3),
    "fc": (3.01, lambda K: 3 * K / 16 + 64),
    "x3f": (3.26, lambda cin: 81 * cin / 16 + cin / 32 + 1),
    "prm_small": (3.01, lambda cf: 81 * cf / 16 + cf / 32 + 2),
    "roi_gemm": (6.51, lambda K: 3 * K / 16),
}


def f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def below(v):
    """the fp32 number next to v towards 0 (nextafter(2^j, 0) of the at-bound inputs)"""
    t = torch.tensor(float(v), dtype=torch.float32)
    return float(torch.nextafter(t, torch.zeros_like(t)))


def scale_of(bound):
    """m3d::f16_scale_of on the bits of the fp32 bound: (s, 1 / s), s a power of two with bound s in [2^14, 2^15)"""
    e = int(torch.tensor([float(bound)], dtype=torch.float32).view(torch.int32)[0]) >> 23 & 255
    f = min(max(268 - e, 2), 252)
    return 2.0 ** (f - 127), 2.0 ** (127 - f)


def cut(a, bound, mutant=None):
    """(hi, lo) of the f16x2 cut of fp32 `a` with the scale of `bound`, both in unscaled units (fp64).  bound: a number, or a tensor that
    broadcasts against a (one bound per group).  mutant: None (the kernels' cut), "scale_up" (the scale exponent one too high),
    "lo_unscaled" (lo cut from the unscaled residual)."""
    a = a.to(torch.float32)
    bt = torch.as_tensor(bound, dtype=torch.float32)
    s = torch.empty(bt.shape, dtype=F64)
    for i, b in enumerate(bt.reshape(-1).tolist()):
        s.view(-1)[i] = scale_of(b)[0]
    if mutant == "scale_up":
        s = s * 2
    s32 = s.to(torch.float32)
    v = a * s32                                               # exact (powers of two)
    h = v.to(torch.float16)
    if mutant == "lo_unscaled":
        l = (a - h.to(torch.float32) / s32).to(torch.float16)
    else:
        l = (v - h.to(torch.float32)).to(torch.float16)
    return h.to(F64) / s, l.to(F64) / s


def emulate(op, a, b, A, B, mutant=None):
    """op(a, b) (bilinear, fp64) as the kernels compute it: h_a h_b + h_a l_b + l_a h_b summed exactly.  mutant: also "hi_only" and
    "drop_hilo" (no h_a l_b)."""
    m = mutant if mutant in ("scale_up", "lo_unscaled") else None
    ah, al = cut(a, A, m)
    bh, bl = cut(b, B, m)
    if mutant == "hi_only":
        return op(ah, bh)
    if mutant == "drop_hilo":
        return op(ah, bh) + op(al, bh)
    return op(ah, bh) + op(ah, bl) + op(al, bh)


def terms(op, a, b):
    """(C, sum|a|, sum|b|, n) of every output: op on |a|, |b| and the non-zero masks"""
    a, b = a.to(F64), b.to(F64)
    na, nb = (a != 0).to(F64), (b != 0).to(F64)
    return op(a.abs(), b.abs()), op(a.abs(), nb), op(na, b.abs()), op(na, nb)


def bound(kernel, k, C, Sa, Sb, n, A, B, y, gain=1.0):
    """E of every output: C, Sa, Sb, n from `terms` (fp64), A / B the operand bounds (numbers or broadcastable tensors), y the fp64
    reference output (with shift / bias), gain |multiplier| applied after the sum (numbers or broadcastable)."""
    c1, nacc = KERNELS[kernel]
    A, B = torch.as_tensor(A, dtype=F64), torch.as_tensor(B, dtype=F64)
    F = C2 * 2.0 ** -39 * (A * Sb + B * Sa) + 2.0 ** -77 * n * A * B
    e = c1 * 2.0 ** -22 * C + F + C3 * nacc(k) * 2.0 ** -24 * (C + F)
    return torch.as_tensor(gain, dtype=F64) * e + 2.0 ** -24 * y.abs()


def inputs(name, xshape, wshape, seed, signed, col=False):
    """(x, w) of an input family, fp32: benign (relu(randn) 3, or randn 3 where signed), heavy (exp(3 randn), random sign where signed),
    outlier<k> (benign + one element, or with col one column of x, at 2^k x the max), quiet (the low half along x scaled by 2^-30),
    at_bound_pow2 / at_bound_below (every input 2^j / the fp32 number below 2^j, every weight +max|w|), zero"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(wshape, generator=g) * 0.2
    if name == "heavy":
        x = torch.exp(3.0 * torch.randn(xshape, generator=g))
        if signed:
            x = x * torch.sign(torch.randn(xshape, generator=g))
        return x, w
    if name.startswith("at_bound"):
        j = int(torch.randint(-20, 20, (1,), generator=g))
        b = 2.0 ** j if name == "at_bound_pow2" else below(2.0 ** j)
        return torch.full(xshape, b, dtype=torch.float32), torch.full(wshape, float(w.abs().max()))
    if name == "zero":
        return torch.zeros(xshape), w
    x = torch.randn(xshape, generator=g)
    x = (x if signed else torch.relu(x)) * 3.0
    if name.startswith("outlier"):
        big = float(x.abs().max()) * 2.0 ** int(name[7:])
        if col:
            x[:, 3] = big
        else:
            x.view(-1)[x.numel() // 3] = big
    elif name == "quiet":
        x[..., : xshape[-1] // 2] *= 2.0 ** -30
    return x, w


# ------------------------------------------------------------------ the ops, bilinear in (a, b), fp64
def linear_op(x, w):
    """x [M, K] @ w[N, K].T"""
    return x @ w.T


def conv3d_op(x, w):
    """'same' 3^3 conv: x [B, cin, D, H, W], w [cout, cin, 3, 3, 3]"""
    return torch.nn.functional.conv3d(x, w, padding=1)


def dgrad_op(g, w):
    """backward-data of a 'same' 3^3 conv with weight w [cout_fwd, cin_fwd, 3, 3, 3] on windows g [P, cout_fwd, n, n, n] (zero outside)"""
    return torch.nn.functional.conv_transpose3d(g, w, padding=1)


# ------------------------------------------------------------------ conv3d_zw: Winograd F(2,3) along z
def zw_operands(x, w):
    """the operands the zw kernel multiplies: V [4, B, pairs, cin, H, W] (fp32 sums of two input planes, zero planes outside the volume)
    and U [4, cout, cin, 3, 3] (transformed in fp64, rounded to fp32)"""
    x = x.to(torch.float32)
    Bn, cin, D, H, W = x.shape
    pairs = (D + 1) // 2
    xp = torch.zeros(Bn, cin, 2 * pairs + 2, H, W, dtype=torch.float32)
    xp[:, :, 1:D + 1] = x
    d = [xp[:, :, k:k + 2 * pairs:2] for k in range(4)]            # d_k of pair j = x[2j - 1 + k]
    V = torch.stack([d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]).transpose(2, 3)
    g = w.to(F64)
    g0, g1, g2 = g[:, :, 0], g[:, :, 1], g[:, :, 2]
    U = torch.stack([g0, 0.5 * (g0 + g1 + g2), 0.5 * (g0 - g1 + g2), g2]).to(torch.float32)
    return V, U


def zw_combine(V, U, D, mode="signed"):
    """out[2j] = M0 + M1 + M2, out[2j + 1] = M1 - M2 - M3 with M_k = the (y, x) conv of V_k with U_k; mode "abs": all four with +
    (the magnitude sums of the contract), V and U given as what op to apply (fp64)"""
    _, Bn, pairs, cin, H, W = V.shape
    M = [torch.nn.functional.conv2d(V[k].reshape(Bn * pairs, cin, H, W), U[k], padding=1).reshape(Bn, pairs, -1, H, W) for k in range(4)]
    if mode == "abs":
        e, o = M[0] + M[1] + M[2], M[1] + M[2] + M[3]
    else:
        e, o = M[0] + M[1] + M[2], M[1] - M[2] - M[3]
    out = torch.stack([e, o], 2).reshape(Bn, 2 * pairs, -1, H, W).transpose(1, 2)
    return out[:, :, :D].contiguous()


def zw_bounds(in_bound, wamax):
    """(A, B) of the zw kernel: f16_scale_of(2 in_max) for V, f16_scale_of(1.5f max|w|) for U (conv3d_zw.hip); in_bound a number, or a
    tensor [W] of one bound per column (strip mode: the bound of the window the column lies in)"""
    A = (torch.as_tensor(in_bound, dtype=torch.float32) * 2).to(F64)
    return (float(A) if A.dim() == 0 else A), f32(1.5 * f32(wamax))


def zw_emulate(x, w, in_bound, mutant=None):
    """the kernel's sum M0 + M1 + M2 / M1 - M2 - M3 with cut operands (fp64, no accumulation error).  mutant as in `emulate`, plus
    "no_v2" (the scale of V from the input bound without the x2 of a two-plane sum)."""
    V, U = zw_operands(x, w)
    A, B = zw_bounds(in_bound, w.abs().max())
    if mutant == "no_v2":
        A, mutant = A / 2, None
    vh, vl = cut(V, A, mutant if mutant in ("scale_up", "lo_unscaled") else None)
    uh, ul = cut(U, B, mutant if mutant in ("scale_up", "lo_unscaled") else None)
    D = x.shape[2]
    if mutant == "hi_only":
        return zw_combine(vh, uh, D)
    out = zw_combine(vh, uh, D) + zw_combine(vl, uh, D)
    return out if mutant == "drop_hilo" else out + zw_combine(vh, ul, D)


def zw_contract(x, w, in_bound, scale=None, shift=None, relu=False, pool=False):
    """(fp64 reference, E, C) of ZwConv3d(w)(x, in_max with largest slot in_bound, scale, shift, relu, pool)"""
    V, U = zw_operands(x, w)
    A, B = zw_bounds(in_bound, w.abs().max())
    D = x.shape[2]
    Va, Ua = V.to(F64).abs(), U.to(F64).abs()
    Vn, Un = (V != 0).to(F64), (U != 0).to(F64)
    C = zw_combine(Va, Ua, D, "abs")
    Sa, Sb, n = zw_combine(Va, Un, D, "abs"), zw_combine(Vn, Ua, D, "abs"), zw_combine(Vn, Un, D, "abs")
    y = conv3d_op(x.to(F64), w.to(F64))
    gain = 1.0
    if scale is not None:
        gain = scale.to(F64).abs().view(1, -1, 1, 1, 1)
        y = y * scale.to(F64).view(1, -1, 1, 1, 1)
    if shift is not None:
        y = y + shift.to(F64).view(1, -1, 1, 1, 1)
    if relu:
        y = torch.relu(y)
    E = bound("zw", x.shape[1], C, Sa, Sb, n, A, B, y, gain)
    if pool:
        mp = torch.nn.functional.max_pool3d
        y, E, C = mp(y, 2, 2), mp(E, 2, 2), mp(C, 2, 2)
    return y, E, C


# ------------------------------------------------------------------ RoIAlign3D as a linear map: out[c][bin] = sum_k f[c][k] M[k][bin]
def _axis_weights(start, binsz, grid, n, P):
    """[P, n] fp64: the weights the P bins of one axis give the n voxels of that axis, summed over the bin's `grid` samples (sample
    positions and 1 - l in fp32 as the reference kernel computes them, roi_align_kernel_3d.cu); 0 for samples outside [-1, n]"""
    f = torch.float32
    Wt = torch.zeros(P, n, dtype=F64)
    for p in range(P):
        for i in range(grid):
            c = torch.tensor(start, dtype=f) + torch.tensor(float(p), dtype=f) * torch.tensor(binsz, dtype=f)
            c = c + (torch.tensor(i + 0.5, dtype=f) * torch.tensor(binsz, dtype=f)) / torch.tensor(float(grid), dtype=f)
            v = float(c)
            if v < -1.0 or v > n:
                continue
            v = max(v, 0.0)
            lo = int(v)
            if lo >= n - 1:
                lo = hi = n - 1
                v = float(lo)
            else:
                hi = lo + 1
            l = float(torch.tensor(v, dtype=f) - torch.tensor(float(lo), dtype=f))
            h = float(torch.tensor(1.0 - l, dtype=f))
            Wt[p, lo] += h
            Wt[p, hi] += l
    return Wt


def roi_align_ref(feat, rois, scale, ratio, P=7, op=None):
    """fp64 RoIAlign3D forward [R, C, P, P, P] (memory order (n, c, ph, pw, ps) as the reference kernel writes it) of feat [B, C, S, H, W]
    with rois [R, 7] (batch, x1, y1, z1, x2, y2, z2); op(f, Wz, Wy, Wx) -> the map on given operands, default the signed sum"""
    f32t = lambda v: torch.tensor(v, dtype=torch.float32)
    B, Cc, S, H, W = feat.shape
    outs = []
    for r in rois.tolist():
        b = int(r[0])
        sw, sh_, ss = (float(f32t(r[i]) * f32t(scale)) for i in (1, 2, 3))
        ew, eh, es = (float(f32t(r[i]) * f32t(scale)) for i in (4, 5, 6))
        bins = [float(f32t(max(float(f32t(e - s)), 1.0)) / f32t(float(P))) for e, s in ((es, ss), (eh, sh_), (ew, sw))]
        Wz = _axis_weights(ss, bins[0], ratio, S, P)
        Wy = _axis_weights(sh_, bins[1], ratio, H, P) / (ratio ** 3)
        Wx = _axis_weights(sw, bins[2], ratio, W, P)
        fb = feat[b].to(F64)
        o = (op or roi_map)(fb, Wz, Wy, Wx)                              # [C, ps, ph, pw]
        outs.append(o.permute(0, 2, 3, 1).reshape(Cc, P, P, P))          # (ph, pw, ps) memory order
    return torch.stack(outs)


def roi_map(f, Wz, Wy, Wx):
    """sum over (z, y, x) of f[c, z, y, x] Wz[ps, z] Wy[ph, y] Wx[pw, x] -> [C, ps, ph, pw]"""
    return torch.einsum("czyx,az,by,dx->cabd", f, Wz, Wy, Wx)


def roi_contract(feat, rois, scale, ratio, A):
    """(fp64 reference, E, C) of roi_align3d_forward(feat, rois, 7, 7, 7, scale, ratio, feat_absmax=A) on the GEMM path (M >= 0, B = 1)"""
    f = feat.to(F64)
    nz = lambda W: (W != 0).to(F64)
    y = roi_align_ref(f, rois, scale, ratio)
    C = roi_align_ref(f.abs(), rois, scale, ratio)
    Sa = roi_align_ref(f.abs(), rois, scale, ratio, op=lambda fb, a, b, c: roi_map(fb, nz(a), nz(b), nz(c)))
    Sb = roi_align_ref((f != 0).to(F64), rois, scale, ratio)
    n = roi_align_ref((f != 0).to(F64), rois, scale, ratio, op=lambda fb, a, b, c: roi_map(fb, nz(a), nz(b), nz(c)))
    return y, bound("roi_gemm", 128, C, Sa, Sb, n, A, 1.0, y), C
