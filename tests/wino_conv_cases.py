"""The case table of the four fp32 Winograd conv kernels, their fp64 references, a NumPy emulation and their error bound.  No tests live
here: tests/test_wino_conv_cases_host.py proves on the CPU, with the library's host queries (m3d_conv3d_wino2_plan,
m3d_conv3d_stem_wino_plan), that the table reaches every production instantiation under the conditions below, that every integer case
is exact and that seeded defects are caught; tests/test_gpu_wino_conv.py runs the table on the GPU.

Kernels and variants
  w24    csrc/conv3d_wino24.hip, F(2x4,3x3), WinoConv3d(two_d=True): variant (4, tile id, K split, mode)
  w22    csrc/conv3d_wino2.hip, F(2x2,3x3), WinoConv3d(two_d=True, local=True): variant (2, tile id, K split, "")
         (family, tile id, K split) is m3d_conv3d_wino2_plan's answer; tile id 32 / 16 / 8 = 64x4x2 / 32x8x2 / 16x16x2 outputs (x, y, z;
         the local family's tile 32 is 64x2x4); only tile 8 splits K.  mode "" | "pool" | "pool+argmax": the fused 2x2x2 pool of the
         default family, whose tile follows forward_pool2's rule - tile 16 below 48 wide, else tile 32 - and never splits K.
  stem   csrc/conv3d_stem_wino.hip, F(2,5) along x: variant (pool, planes 4 | 8) - m3d_conv3d_stem_wino_plan's planes per workgroup, tile
         64 x 8 x planes.  The release library plans 8 only from 1024 workgroups of 8 planes on (beyond the cost cap): the 8-plane cases
         run through the tuning library's tune_stem option and are the 4-plane cases' shapes.
  w23x   csrc/conv3d_wino.hip, F(2,3) along x, WinoConv3d(two_d=False): variant by m3d_conv3d_wino_forward's rule (W23X_RULE below)
             "w48"    width >= 48               64x2x4 outputs, 64 output channels per workgroup, chunks of 4 input channels
             "w24c64" width 24..47, cout >= 64  32x4x4, 32 output channels, chunks of 8
             "w24"    width 24..47, cout < 64   32x4x2, 64 output channels, chunks of 4 split over two wave groups (channels 0, 1 | 2, 3)
             "pool"   fused pool (width >= 48)  64x4x2, 64 output channels, chunks of 4

Conditions (each holds for at least one case of every variant; LEAD holds one case per variant with all that the variant admits)
  ragged  >= 2 tiles along z, y and x, each with a non-zero remainder
  chunks  cin % chunk != 0 with an odd cin among them, >= 2 chunks (not the stem: one input channel)
  couts   cout % 32 != 0 and >= 2 cout tiles ("w24": cout < 64 is one tile of 64, half empty); an odd number of 32-blocks per kernel at
          least once (the packs pad the blocks to pairs)
  batch   batch 2
  quads   over the un-pooled cases of each 2-D (family, tile), W % 4 takes all of 0, 1, 2, 3
  order   per 2-D family one grid that is no multiple of 8 and one case with >= 5 z tiles, tiles_z % 4 != 0; w24: one case with more than
          16 x tiles (the x-slow tile order)
  splits  K splits 1, 2, 3, 5 (cin 33: 9 chunks in slices of 2, the last slice one chunk) and 8 on tile 8, both families; a single tile
  cost    2 * k^3 * B * cin * cout * D * H * W <= 0.5 GFLOP

Exactness recipe (test_exact_on_integers).  Inputs are small integers, weights integer multiples of UNIT[kernel]; then every transformed
weight is an integer that the pack kernel delivers exactly:
  w22   wino2_pack_kernel, fp32: col = 0.5f * (a +- b + c) of multiples of 4 is an even integer (sums of small integers are exact in
        fp32, a product with 0.5 is exact), then 0.5f * (col0 +- col1 + col2) of even integers is an integer.  UNIT 4.
  w23x  wino_pack_kernel, fp32: 0.5f * (g0 +- g1 + g2) of multiples of 2.  UNIT 2.
  w24   wino24_pack_kernel, double: col = 0.5 * (a +- b + c) of multiples of 48 is a multiple of 24 (exact); along x 0.25 * g0 is exact;
        s = g0 +- g1 + g2 and t = g0 +- 2 g1 + 4 g2 are multiples of 24 (exact sums), and the kernel multiplies them with the DOUBLES
        r6 = fl(1/6), r24 = fl(1/24).  1/6 = 2^-3 * 4/3 and 1/24 = 2^-5 * 4/3; 4/3 = 1.0101...b is cut after 52 fraction bits with a
        remainder of 2^-52 / 3 < half an ulp, so r = (1 - 2^-54) / 6 resp. / 24 exactly.  r6 * s = (s / 6) (1 - 2^-54): s / 6 = 4k is an
        integer below 2^24, the product misses it by 4|k| 2^-54 < ulp(4k) / 2 = 2^(e - 53) (2^e <= 4|k| < 2^(e+1)), so the double
        product rounds to 4k; likewise r24 * t = t / 24.  The cast to float of an integer below 2^24 is exact.  UNIT 48.
  stem  stem_wino_pack4_kernel, double: g0 / 4, sums / 6 and / 24 of multiples of 24 - exact sums, and an IEEE division whose exact
        quotient is an integer returns it.  UNIT 24.
Input and inverse transforms have integer coefficients (+-1, 2, 4, 5, 8), so every intermediate of kernel and emulation is an integer of
magnitude at most wino_abs (below), and every fp32 summation order - the MFMA chains, split-K slices, the reduce kernel - is exact while
wino_abs < 2^24.  The epilogue's scale is a power of two in [1/2, 4] and its shift an integer in [-8, 8]: exact while
4 * wino_abs + 8 < 2^23 (int_ranges picks x in [-2, 2] or [-1, 1] and weights in UNIT * [-2, 2] or [-1, 1] so that this holds).

wino_abs = |A^T| [ (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A| summed over input channels and the direct taps (z; y too for stem and w23x),
patches aligned as the kernels align them: from x = 0 and y = 0, in steps of 4 (w24) or 2 along x and 2 along y, zeros outside the volume.

Error bound of the random-data tests, per element (derived, not fitted):
    |got - y| <= C3 * n * 2^-24 * wino_abs + 2^-24 * |y|          (with the epilogue: wino_abs * |scale| + |shift| for wino_abs)
Every rounding of an intermediate v costs at most 2^-24 |v|, and what |v| can contribute to an output is bounded by the same expression
with absolute values, i.e. by wino_abs; n counts the roundings on the longest path into one output (n_roundings), read from the kernels:
    w24   1 weight (double -> float) + 1 y input transform (U -+ V) + 2 x input transform (fma in fma; sum of two fmas) + 3 * cin
          accumulated products (MFMA chain over dz x channel) + 3 x inverse (q3 = d12 + 8 d34 + acc5) + 2 y inverse ((q0 + q1) + q2)
    w22   4 weight (two fp32 sums of three, twice) + 1 + 1 input transforms + 3 * cin + 2 x inverse (a0 + a1 + a2) + 2 y inverse
          (half 1's -p0 - p1, then half 0's sum with it)
    w23x  2 weight (fp32 sum of three) + 1 input transform + 9 * cin + 2 inverse; "w24" + 1: the two wave groups' halves are added
    stem  1 weight + 2 input transform + 25 accumulated products + 4 inverse (m0 + m1 + m2 + m3 + m4)
    + (K split - 1) additions of the reduce kernel, + 2 for the epilogue's product and sum where one is applied
C3 = 2 is the allowance of tests/f16x2_contract.py for an accumulate that truncates.  The last term is the rounding of the stored result.

Largest measured |got - y| / bound per variant (MI355X; tests/test_gpu_wino_conv.py prints them with pytest -s, one line per case and the
worst per variant at the end of the module) - far below 1, as a worst-case bound on random data must be; every exact test passed:
    w24   tile 32  0.0079 (pool 0.0047, pool + arg-max 0.0047)   tile 16  0.0063 (pool 0.0032, pool + arg-max 0.0030)
          tile 8, K split 1 / 2 / 3 / 4 / 5 / 8   0.0075 / 0.0058 / 0.0018 / 0.0017 / 0.0003 / 0.0006
    w22   tile 32  0.0092   tile 16  0.0090   tile 8, K split 1 / 2 / 3 / 4 / 5 / 8   0.0119 / 0.0073 / 0.0047 / 0.0024 / 0.0006 / 0.0009
    stem  4 planes 0.0136 (pool 0.0102)   8 planes 0.0136 (pool 0.0102)
    w23x  w48 0.0115   w24c64 0.0055   w24 0.0077   pool 0.0095
The NumPy emulation's own largest ratio on the same operands is 0.0148 (tests/test_wino_conv_cases_host.py prints it per kernel).
"""
import collections

import numpy as np
import torch

from direct_conv_cases import integers, conv64, pool_gather  # noqa: F401  (shared with the direct-conv tests, not copied)

F64 = torch.float64
CAP_FLOP = 0.5e9
C3 = 2.0                      # tests/f16x2_contract.py: the allowance for a truncating accumulate
UNIT = {"w22": 4, "w24": 48, "stem": 24, "w23x": 2}
KSIZE = {"w22": 3, "w24": 3, "stem": 5, "w23x": 3}

Case = collections.namedtuple("Case", "kernel variant batch cin cout D H W pool argmax")


def W23X_RULE(cout, width, pool):
    """m3d_conv3d_wino_forward / _forward_pool2: the instantiation by width and cout"""
    if pool:
        return "pool" if width >= 48 else None
    if width >= 48:
        return "w48"
    if width >= 24:
        return "w24c64" if cout >= 64 else "w24"
    return None


def _w24(tile, ks, batch, cin, cout, D, H, W, mode=""):
    return Case("w24", (4, tile, ks, mode), batch, cin, cout, D, H, W, mode != "", mode == "pool+argmax")


def _w22(tile, ks, batch, cin, cout, D, H, W):
    return Case("w22", (2, tile, ks, ""), batch, cin, cout, D, H, W, False, False)


def _stem(planes, batch, cout, D, H, W, pool=False):
    return Case("stem", (pool, planes), batch, 1, cout, D, H, W, pool, False)


def _w23x(batch, cin, cout, D, H, W, pool=False):
    return Case("w23x", W23X_RULE(cout, W, pool), batch, cin, cout, D, H, W, pool, False)


# one case per variant that is ragged on every axis, has an odd cin with a partial last chunk, a partial last cout tile and batch 2
LEAD = (
    _w24(32, 1, 2, 5, 70, 13, 5, 65),             # 7 z tiles; 2 * 2 * 7 * 3 = 84 workgroups per item: no multiple of 8
    _w24(16, 1, 2, 5, 40, 11, 17, 33),
    _w24(8, 1, 2, 5, 70, 13, 17, 18),             # 168 tiles > 128: K unsplit on the split-capable tile; 7 z tiles, 84 workgroups
    _w24(8, 2, 2, 5, 40, 3, 17, 17),
    _w24(8, 3, 2, 9, 40, 3, 17, 19),
    _w24(8, 5, 2, 33, 40, 3, 17, 20),             # 9 chunks in slices of 2: the fifth slice is one chunk, its one channel
    _w24(8, 8, 2, 29, 40, 3, 17, 17),
    _w24(32, 1, 2, 5, 70, 5, 7, 70, "pool"),
    _w24(32, 1, 2, 5, 70, 5, 7, 70, "pool+argmax"),
    _w24(16, 1, 2, 5, 40, 5, 11, 37, "pool"),
    _w24(16, 1, 2, 5, 40, 5, 11, 37, "pool+argmax"),
    _w22(32, 1, 2, 5, 70, 13, 3, 65),             # 64x2x4: 4 z tiles, 2 y tiles
    _w22(16, 1, 2, 5, 40, 11, 17, 33),
    _w22(8, 1, 2, 5, 70, 13, 17, 18),
    _w22(8, 2, 2, 5, 40, 3, 17, 17),
    _w22(8, 3, 2, 9, 40, 3, 17, 19),
    _w22(8, 5, 2, 33, 40, 3, 17, 20),
    _w22(8, 8, 2, 29, 40, 3, 17, 17),
    _stem(4, 2, 40, 11, 13, 75),                  # 3 z tiles of 4 (2 of 8), 2 y tiles, 2 x tiles; 40 channels: a block of 32 and one of 8
    _stem(8, 2, 40, 11, 13, 75),
    _stem(4, 2, 40, 11, 13, 75, pool=True),
    _stem(8, 2, 40, 11, 13, 75, pool=True),
    _w23x(2, 5, 70, 7, 5, 70),
    _w23x(2, 13, 70, 7, 7, 37),                   # chunks of 8: 8 + 5
    _w23x(2, 7, 40, 5, 7, 37),                    # the second chunk's wave groups hold channels (4, 5) and (6, none)
    _w23x(2, 5, 70, 5, 7, 70, pool=True),
)

# further edges: the other widths modulo 4, full chunks and cout tiles, one tile, batch 1, thresholds, the x-slow tile order
MORE = (
    _w24(32, 1, 1, 8, 32, 3, 9, 1100),            # 18 x tiles: x-slow order; W % 4 = 0
    _w24(32, 1, 1, 4, 64, 8, 8, 66),               # one full chunk (more would split K on tile 8 instead)
    _w24(32, 1, 1, 4, 33, 4, 8, 127),
    _w24(16, 1, 1, 4, 64, 8, 16, 34),
    _w24(16, 1, 1, 4, 33, 6, 16, 35),
    _w24(16, 1, 2, 4, 32, 8, 16, 32),             # full tiles, a full chunk, a full cout block
    _w24(8, 2, 1, 8, 32, 2, 16, 16),              # a single tile, two full chunks
    _w24(8, 4, 2, 13, 40, 3, 17, 17),
    _w24(8, 1, 1, 3, 20, 22, 40, 23),             # one chunk: nothing to split; 11 z tiles; 3 * 11 * 2 = 66 workgroups
    _w24(32, 1, 1, 8, 33, 4, 8, 128, "pool+argmax"),      # even pooled width: paired stores
    _w24(16, 1, 1, 8, 33, 4, 8, 24, "pool+argmax"),       # W at the pool's lower threshold
    _w24(16, 1, 1, 4, 32, 4, 8, 47, "pool"),
    _w24(32, 1, 1, 4, 32, 4, 8, 48, "pool"),
    _w22(32, 1, 1, 4, 64, 8, 8, 66),
    _w22(32, 1, 1, 4, 33, 8, 4, 127),
    _w22(32, 1, 1, 4, 32, 9, 4, 128),
    _w22(16, 1, 1, 4, 64, 8, 16, 34),
    _w22(16, 1, 1, 4, 33, 6, 16, 35),
    _w22(16, 1, 2, 4, 32, 8, 16, 32),
    _w22(8, 2, 1, 8, 32, 2, 16, 16),
    _w22(8, 4, 2, 13, 40, 3, 17, 17),
    _w22(8, 1, 1, 3, 20, 22, 40, 23),
    _stem(4, 1, 32, 4, 8, 64),                    # exactly one tile
    _stem(4, 1, 33, 5, 9, 33),                    # W just over the kernel's lower limit, one channel in the second block
    _stem(4, 1, 20, 6, 10, 66, pool=True),
    _stem(4, 1, 70, 3, 5, 40),                    # three blocks of channels
    _w23x(1, 8, 64, 4, 2, 64),                    # exactly one tile
    _w23x(1, 6, 65, 5, 3, 67),                    # odd width: unpaired stores
    _w23x(1, 8, 64, 4, 4, 24),                    # W and cout at the thresholds
    _w23x(1, 16, 96, 5, 6, 47),
    _w23x(1, 8, 63, 2, 4, 24),
    _w23x(1, 4, 20, 3, 5, 47),
    _w23x(1, 8, 64, 4, 4, 48, pool=True),
    _w23x(1, 6, 33, 6, 8, 67, pool=True),
)

CASES = LEAD + MORE


def case_id(c):
    v = "-".join(str(int(t) if isinstance(t, bool) else t) for t in c.variant if t != "") if isinstance(c.variant, tuple) else c.variant
    return "%s-%s-b%d-%dto%d-%dx%dx%d" % (c.kernel, v, c.batch, c.cin, c.cout, c.D, c.H, c.W)


def flop(c):
    return 2.0 * KSIZE[c.kernel] ** 3 * c.batch * c.cin * c.cout * c.D * c.H * c.W


def tile_of(c):
    """(tile_x, tile_y, tile_z, output channels per workgroup, input channels per chunk) of the case's variant"""
    if c.kernel in ("w24", "w22"):
        fam, tile = c.variant[0], c.variant[1]
        xyz = {32: (64, 4, 2) if fam == 4 else (64, 2, 4), 16: (32, 8, 2), 8: (16, 16, 2)}[tile]
        return xyz + (32, 4)
    if c.kernel == "stem":
        return (64, 8, c.variant[1], 32, 1)
    return {"w48": (64, 2, 4, 64, 4), "w24c64": (32, 4, 4, 32, 8), "w24": (32, 4, 2, 64, 4), "pool": (64, 4, 2, 64, 4)}[c.variant]


def ksplit_of(c):
    return c.variant[2] if c.kernel in ("w24", "w22") else 1


def slices_of(c):
    """the input channels of every partial sum, in the order the partial sums are added"""
    if c.kernel == "w23x" and c.variant == "w24":
        return [[ci for ci in range(c.cin) if ci % 4 < 2], [ci for ci in range(c.cin) if ci % 4 >= 2]]
    ks = ksplit_of(c)
    if ks == 1:
        return [list(range(c.cin))]
    nchunk = (c.cin + 3) // 4
    cps = (nchunk + ks - 1) // ks                 # plan_splitk: chunks per slice; the last slice takes what is left
    out = [list(range(4 * cps * s, min(c.cin, 4 * cps * (s + 1)))) for s in range(ks)]
    assert all(out) and sum(len(s) for s in out) == c.cin
    return out


def n_roundings(c, epilogue=False):
    """roundings on the longest path into one output element (the module docstring, term by term)"""
    n = {"w24": 1 + 1 + 2 + 3 * c.cin + 3 + 2, "w22": 4 + 1 + 1 + 3 * c.cin + 2 + 2, "w23x": 2 + 1 + 9 * c.cin + 2, "stem": 1 + 2 + 25 + 4}[c.kernel]
    n += len(slices_of(c)) - 1
    return n + (2 if epilogue else 0)


def bound(c, y, wabs, scale=None, shift=None):
    """the per-element error bound; y = the fp64 result, wabs = wino_abs (of the conv; scale / shift: the epilogue applied to reach y)"""
    a = wabs
    if scale is not None:
        a = wabs * scale.to(F64).abs().view(1, -1, 1, 1, 1) + shift.to(F64).abs().view(1, -1, 1, 1, 1)
    return C3 * n_roundings(c, scale is not None) * 2.0 ** -24 * a + 2.0 ** -24 * y.abs()


# ------------------------------------------------------------------ transforms: matrices (wino_abs) and the kernels' formulas (emulate)
_BT23 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=np.float64)
_G23 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=np.float64)
_AT23 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=np.float64)
_BT6 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                 [0, 4, 0, -5, 0, 1]], dtype=np.float64)
_G43 = np.array([[6, 0, 0], [-4, -4, -4], [-4, 4, -4], [1, 2, 4], [1, -2, 4], [0, 0, 24]], dtype=np.float64) / 24.0
_AT43 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)
_G25 = np.array([[6, 0, 0, 0, 0], [-4, -4, -4, -4, -4], [-4, 4, -4, 4, -4], [1, 2, 4, 8, 16], [1, -2, 4, -8, 16], [0, 0, 0, 0, 24]],
                dtype=np.float64) / 24.0
_AT25 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1]], dtype=np.float64)
# kernel -> x transform (B^T, G, A^T), outputs per patch along x, left padding; y transform (F(2,3)) or None: direct taps along y
_XFORM = {"w24": (_BT6, _G43, _AT43, 4, 1), "w22": (_BT23, _G23, _AT23, 2, 1), "w23x": (_BT23, _G23, _AT23, 2, 1),
          "stem": (_BT6, _G25, _AT25, 2, 2)}
_Y_WINO = {"w24": True, "w22": True, "w23x": False, "stem": False}


def _np(t, dtype=np.float64):
    return np.ascontiguousarray(t.detach().cpu().numpy().astype(dtype))


def _padded(kernel, x, defect=None):
    """x [B, C, D, H, W] with the zeros (or, as a seeded defect, the wrong values) the kernel's patches see around it: z by the direct
    taps, y by one row and up to whole patches (Winograd along y) or by the direct taps, x from -pad to the end of the last patch"""
    B, C, D, H, W = x.shape
    k = KSIZE[kernel]
    bt, _, _, m, px = _XFORM[kernel]
    alpha = bt.shape[0]
    tx = -(-W // m)
    ty = -(-H // 2)
    pz = k // 2
    hp = 2 * (ty - 1) + 4 if _Y_WINO[kernel] else H + 2 * (k // 2)
    py = 1 if _Y_WINO[kernel] else k // 2
    xp = np.zeros((B, C, D + 2 * pz, hp, m * (tx - 1) + alpha), dtype=x.dtype)
    xp[:, :, pz:pz + D, py:py + H, px:px + W] = x
    if defect == "drop_last_x":                   # a mask one element short at the last column: the last channel loses x = W - 1
        xp[:, C - 1, :, :, px + W - 1] = 0
    if defect == "halo_wrap":                     # x = -1 unmasked: the element one float before the row, i.e. the previous row's last
        flat = x.reshape(B, -1)
        lin = np.arange(C * D * H).reshape(C, D, H) * W - 1
        prev = np.where(lin >= 0, flat[:, np.maximum(lin, 0)], 0).astype(x.dtype)
        xp[:, :, pz:pz + D, py:py + H, px - 1] = prev
    return xp, tx, ty


def _take(a, axis, step, count, width):
    """patches along `axis`: the axis becomes (count, width), patch t = elements step * t .. step * t + width - 1"""
    idx = step * np.arange(count)[:, None] + np.arange(width)[None, :]
    return np.take(a, idx, axis=axis)


def _gemm(u, v, chans, D, dtype):
    """sum over the channels `chans` and the direct taps: u [O, C, taps_z(, taps_y)], v [B, C, Zp, Y(p), X] -> [B, O, D, Y, X]"""
    acc = None
    Hy = v.shape[3] - (u.shape[3] - 1 if u.ndim == 4 else 0)
    for dz in range(u.shape[2]):
        for dy in range(u.shape[3] if u.ndim == 4 else 1):
            a = u[:, chans, dz, dy] if u.ndim == 4 else u[:, chans, dz]
            b = v[:, chans, dz:dz + D, dy:dy + Hy]
            t = np.tensordot(a.astype(dtype), b, axes=([1], [1]))        # [O, B, D, Y, X]
            acc = t if acc is None else acc + t
    return np.moveaxis(acc, 0, 1)


def _assemble(rows, H, W):
    """rows[r][j]: [B, O, D, Ty, Tx] (or rows[0][j]: [B, O, D, H, Tx]) -> [B, O, D, H, W]"""
    y = np.stack([np.stack(r, axis=-1) for r in rows], axis=4)           # [B, O, D, Ty, R, Tx, J]
    B, O, D, Ty, R, Tx, J = y.shape
    return y.reshape(B, O, D, Ty * R, Tx * J)[:, :, :, :H, :W]


def _wino_matrix(c, x, w, absolute):
    """the kernel's Winograd algorithm in fp64 through its transform matrices (absolute: every matrix and operand by absolute value)"""
    f = np.abs if absolute else (lambda a: a)
    bt, g, at, m, _ = (f(a) if isinstance(a, np.ndarray) else a for a in _XFORM[c.kernel])
    xp, tx, ty = _padded(c.kernel, f(_np(x)))
    wn = f(_np(w))
    D, H, W = c.D, c.H, c.W
    d = _take(xp, 4, m, tx, bt.shape[0])                                  # [B, C, Zp, Yp, Tx, alpha]
    v = np.einsum("bczyxj,kj->kbczyx", d, bt)
    u = np.einsum("ocdyj,kj->kocdy", wn, g)                               # [xi, O, C, dz, dy]
    if _Y_WINO[c.kernel]:
        v = np.einsum("kbczyix,ei->ekbczyx", _take(v, 4, 2, ty, 4), f(_BT23))
        u = np.einsum("kocdy,ey->ekocd", u, f(_G23))
        mm = [[_gemm(u[e, k], v[e, k], slice(None), D, np.float64) for k in range(bt.shape[0])] for e in range(4)]
        q = [[sum(at[j, k] * mm[e][k] for k in range(bt.shape[0])) for j in range(m)] for e in range(4)]
        rows = [[sum(f(_AT23)[r, e] * q[e][j] for e in range(4)) for j in range(m)] for r in range(2)]
        return torch.from_numpy(_assemble(rows, H, W).copy())
    mm = [_gemm(u[k], v[k], slice(None), D, np.float64) for k in range(bt.shape[0])]
    rows = [[sum(at[j, k] * mm[k] for k in range(bt.shape[0])) for j in range(m)]]
    y = np.stack(rows[0], axis=-1)                                        # [B, O, D, H, Tx, J]
    return torch.from_numpy(y.reshape(y.shape[:4] + (-1,))[..., :W].copy())


def wino_abs(c, x, w):
    """|A^T| [ (|G| |g| |G^T|) .* (|B^T| |d| |B|) ] |A| summed over input channels and direct taps, fp64 [B, cout, D, H, W]: the largest
    magnitude any intermediate of the kernel can contribute to each output (the exactness condition and the error bound's scale)"""
    return _wino_matrix(c, x, w, True)


def wino_plain(c, x, w):
    """the same expression with the matrices as they are: the conv itself (the host test holds it against conv64)"""
    return _wino_matrix(c, x, w, False)


def _fma(a, b, c):
    """a * b + c with one rounding (a: a small integer constant)"""
    if c.dtype == np.float32:
        return (np.float64(a) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return a * b + c


def _in23(d):
    return [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]


def _in6(c, defect=None):
    """B^T d of F(4,3) / F(2,5) as conv3d_wino24_kernel's and conv3d_stem_wino4_kernel's `transform` write it"""
    t0, t1 = _fma(-4.0, c[2], c[4]), _fma(-4.0, c[1], c[3])
    t2, t3 = c[4] - c[2], c[3] - c[1]
    five = -4.0 if defect == "coef5" else -5.0
    return [_fma(4.0, c[0], _fma(five, c[2], c[4])), t0 + t1, t0 - t1, _fma(2.0, t3, t2), _fma(-2.0, t3, t2),
            _fma(4.0, c[1], _fma(-5.0, c[3], c[5]))]


def packed_weights(c, w, dtype):
    """the transformed weights [xi, O, C, dz, dy | eta] as the kernel's pack computes them; dtype float32: rounded to fp32 as the pack
    rounds them (w22, w23x: fp32 arithmetic; w24, stem: double arithmetic, then the cast); float64: not rounded at all"""
    if c.kernel in ("w22", "w23x"):
        g = _np(w, dtype)
        half = dtype(0.5)

        def g23(a, b, cc):
            return [a, half * (a + b + cc), half * (a - b + cc), cc]
        if c.kernel == "w22":                     # along y first (dy = axis 3), then along x
            col = np.stack(g23(g[:, :, :, 0], g[:, :, :, 1], g[:, :, :, 2]), axis=3)          # [O, C, dz, eta, dx]
            return np.stack(g23(col[..., 0], col[..., 1], col[..., 2]), axis=0)
        return np.stack(g23(g[..., 0], g[..., 1], g[..., 2]), axis=0)                        # [xi, O, C, dz, dy]
    g = _np(w, np.float64)
    if c.kernel == "w24":
        a, b, cc = g[:, :, :, 0], g[:, :, :, 1], g[:, :, :, 2]
        col = np.stack([a, 0.5 * (a + b + cc), 0.5 * (a - b + cc), cc], axis=3)              # [O, C, dz, eta, dx]
        g0, g1, g2 = col[..., 0], col[..., 1], col[..., 2]
        r6, r24 = 1.0 / 6.0, 1.0 / 24.0
        u = [0.25 * g0, -r6 * (g0 + g1 + g2), -r6 * (g0 - g1 + g2), r24 * (g0 + 2.0 * g1 + 4.0 * g2), r24 * (g0 - 2.0 * g1 + 4.0 * g2), g2]
    else:
        g0, g1, g2, g3, g4 = (g[..., i] for i in range(5))
        u = [g0 / 4.0, -(g0 + g1 + g2 + g3 + g4) / 6.0, -(g0 - g1 + g2 - g3 + g4) / 6.0, (g0 + 2.0 * g1 + 4.0 * g2 + 8.0 * g3 + 16.0 * g4) / 24.0,
             (g0 - 2.0 * g1 + 4.0 * g2 - 8.0 * g3 + 16.0 * g4) / 24.0, g4]
    u = np.stack(u, axis=0)
    return u.astype(np.float32).astype(dtype) if dtype == np.float32 else u


DEFECTS = ("drop_last_x", "coef5", "short_slice", "halo_wrap", "shift_per_slice")


def defect_applies(c, defect):
    if defect == "coef5":
        return c.kernel in ("w24", "stem")                                # the kernels with the six-point input transform
    if defect == "short_slice":
        return c.kernel != "stem" and (c.cin + tile_of(c)[4] - 1) // tile_of(c)[4] >= 2
    if defect == "shift_per_slice":
        return ksplit_of(c) > 1
    return True


def emulate(c, x, w, dtype=np.float32, scale=None, shift=None, relu=False, defect=None):
    """The kernel's algorithm in NumPy at `dtype`: its input transforms as its code writes them, its packed weights (rounded to fp32 at
    float32), one partial sum per K slice - transformed back on its own and added in the reduce kernel's order - then the epilogue.  Returns
    the un-pooled [B, cout, D, H, W] (the fused pools are max_pool3d of it).  defect: one of DEFECTS, a seeded fault."""
    assert defect is None or defect_applies(c, defect)
    kernel = c.kernel
    bt, _, _, m, _ = _XFORM[kernel]
    alpha = bt.shape[0]
    xp, tx, ty = _padded(kernel, _np(x, dtype), defect)
    u = packed_weights(c, w, dtype)
    D, H, W = c.D, c.H, c.W
    d = _take(xp, 4, m, tx, alpha)                                        # [B, C, Zp, Yp, Tx, alpha]
    sl = slices_of(c)
    if defect == "short_slice":
        cc = tile_of(c)[4]
        last = sl[-1]
        keep = [ci for ci in last if ci // cc < last[-1] // cc] if kernel != "w23x" or c.variant != "w24" else [ci for ci in last if ci // 4 < (c.cin - 1) // 4]
        sl = sl[:-1] + [keep]
    parts = []
    if _Y_WINO[kernel]:
        dy = _take(d, 3, 2, ty, 4)                                        # [B, C, Zp, Ty, 4, Tx, alpha]
        rows = _in23([dy[:, :, :, :, i] for i in range(4)])               # y transform first: [B, C, Zp, Ty, Tx, alpha] per eta
        v = [(_in6([r[..., j] for j in range(6)], defect) if alpha == 6 else _in23([r[..., j] for j in range(4)])) for r in rows]
        for chans in sl:
            if not chans:
                parts.append(np.zeros((c.batch, c.cout, D, H, W), dtype=dtype))
                continue
            a = [[_gemm(u[k][:, :, :, e], v[e][k], chans, D, dtype) for k in range(alpha)] for e in range(4)]
            if alpha == 6:
                q = []
                for e in range(4):
                    d12, s12, d34, s34 = a[e][1] - a[e][2], a[e][1] + a[e][2], a[e][3] - a[e][4], a[e][3] + a[e][4]
                    two, four, eight = dtype(2), dtype(4), dtype(8)
                    q.append([a[e][0] + s12 + s34, d12 + two * d34, s12 + four * s34, d12 + eight * d34 + a[e][5]])
            else:
                q = [[a[e][0] + a[e][1] + a[e][2], a[e][1] - a[e][2] - a[e][3]] for e in range(4)]
            out = [[(q[0][j] + q[1][j]) + q[2][j] for j in range(m)], [(q[1][j] - q[2][j]) - q[3][j] for j in range(m)]]
            parts.append(_assemble(out, H, W))
    else:
        cols = [d[..., j] for j in range(alpha)]
        v = _in6(cols, defect) if alpha == 6 else _in23(cols)
        for chans in sl:
            if not chans:
                parts.append(np.zeros((c.batch, c.cout, D, H, W), dtype=dtype))
                continue
            a = [_gemm(u[k], v[k], chans, D, dtype) for k in range(alpha)]
            if alpha == 6:
                two = dtype(2)
                out = [[a[0] + a[1] + a[2] + a[3] + a[4], (a[1] - a[2]) + two * (a[3] - a[4]) + a[5]]]
            else:
                out = [[a[0] + a[1] + a[2], a[1] - a[2] - a[3]]]
            yv = np.stack(out[0], axis=-1)
            parts.append(yv.reshape(yv.shape[:4] + (-1,))[..., :W])
    y = parts[0]
    for p in parts[1:]:
        y = y + p
    assert y.dtype == dtype and y.shape == (c.batch, c.cout, D, H, W)
    if scale is not None:
        sh = _np(shift, dtype) * dtype(len(parts) if defect == "shift_per_slice" else 1)
        y = y * _np(scale, dtype).reshape(1, -1, 1, 1, 1) + sh.reshape(1, -1, 1, 1, 1)
    if relu:
        y = np.maximum(y, dtype(0))
    return torch.from_numpy(np.ascontiguousarray(y))


# ------------------------------------------------------------------ operands
def _unit_abs(kernel):
    """wino_abs per input channel at |x| = 1 and |w| = 1 everywhere, in the interior of a volume"""
    shape = {"w24": (1, 1, 3, 6, 12), "w22": (1, 1, 3, 6, 6), "w23x": (1, 1, 3, 3, 6), "stem": (1, 1, 5, 5, 36)}[kernel]   # a patch with no zero
    k = KSIZE[kernel]
    variant = {"w24": (4, 8, 1, ""), "w22": (2, 8, 1, ""), "w23x": "w24", "stem": (False, 4)}[kernel]
    c = Case(kernel, variant, 1, 1, 1, shape[2], shape[3], shape[4], False, False)
    return float(wino_abs(c, torch.ones(shape), torch.ones((1, 1, k, k, k))).max())


_UNIT_ABS = {}


def int_ranges(c):
    """(largest |x|, largest |w| / UNIT) of the case's integer operands: the widest of (2, 2), (2, 1), (1, 1) with
    4 * wino_abs + 8 < 2^23 for any data in the range (the module docstring)"""
    if c.kernel not in _UNIT_ABS:
        _UNIT_ABS[c.kernel] = _unit_abs(c.kernel)
    for xm, wm in ((2, 2), (2, 1), (1, 1)):
        if 4.0 * _UNIT_ABS[c.kernel] * c.cin * xm * wm * UNIT[c.kernel] + 8 < 2.0 ** 23:
            return xm, wm
    raise AssertionError("no exact integer range for %s" % (c,))


def integer_operands(c):
    """x, w integer-valued (w in multiples of UNIT), non-zero at the first and last element of every batch item and of the weight: the
    shifted first quad and the last masked quad carry data.  Cases of one shape share their operands."""
    gen = torch.Generator().manual_seed(c.cin * 1000003 + c.cout * 1009 + c.D * 101 + c.H * 11 + c.W)
    xm, wm = int_ranges(c)
    k = KSIZE[c.kernel]
    x = integers((c.batch, c.cin, c.D, c.H, c.W), -xm, xm, gen)
    w = integers((c.cout, c.cin, k, k, k), -wm, wm, gen)
    x[:, 0, 0, 0, 0], x[:, -1, -1, -1, -1] = float(xm), -float(xm)
    w.view(-1)[0], w.view(-1)[-1] = float(wm), -float(wm)
    return x, w * UNIT[c.kernel]


def epilogue_operands(c, negative=False):
    """power-of-two scale (negative: some of them negated), integer shift: every step of the epilogue is exact"""
    gen = torch.Generator().manual_seed(7 + c.cout)
    scale = 2.0 ** torch.randint(-1, 3, (c.cout,), generator=gen).to(torch.float32)
    if negative:
        scale = scale * (1 - 2 * torch.randint(0, 2, (c.cout,), generator=gen)).to(torch.float32)
    return scale, integers((c.cout,), -8, 8, gen)


def random_operands(c):
    """N(0, 1) inputs, He-scaled weights, scales in [0.5, 1.5) (the stem: [-0.3, 0.7), negative among them), N(0, 1) shifts"""
    gen = torch.Generator().manual_seed(c.cin * 1000003 + c.cout * 1009 + c.D * 101 + c.H * 11 + c.W + 1)
    k = KSIZE[c.kernel]
    x = torch.randn((c.batch, c.cin, c.D, c.H, c.W), generator=gen)
    w = torch.randn((c.cout, c.cin, k, k, k), generator=gen) * (2.0 / (k ** 3 * c.cin)) ** 0.5
    scale = torch.rand((c.cout,), generator=gen) + (-0.3 if c.kernel == "stem" else 0.5)
    return x, w, scale, torch.randn((c.cout,), generator=gen)


def epilogue64(conv, scale, shift, relu=True):
    v = conv * scale.to(F64).view(1, -1, 1, 1, 1) + shift.to(F64).view(1, -1, 1, 1, 1)
    return torch.relu(v) if relu else v
