"""The case table of the direct fp32 conv family (csrc/conv3d.hip), its fp64 references and its error bound.  No tests live here:
tests/test_direct_conv_cases_host.py proves on the CPU, with m3d_conv3d_direct_plan, that the table reaches every production
instantiation under the conditions below; tests/test_gpu_direct_conv.py runs it.

Variant ids (m3d_conv3d_direct_plan; conv3d_mfma_kernel<CC, XB, ROWS, NCB[, KS]>, voxel tile x*y*z):

     0 <4,32,4,1>   32x4x4      1 <4,16,2,1>  16x4x4       2 <4,8,2,1>       8x8x4      (k = 3, cout <= 32)
     3 <2,32,4,2>   32x4x4      4 <8,32,2,2,KS2> 32x2x4    5 <8,32,1,2,KS2> 32x1x4      6 <2,32,2,2> 32x2x4     7 <4,32,1,2> 32x1x4
     8 <4,16,2,2>   16x4x4      9 <4,16,1,1>  16x2x4      10 <8,16,1,1,KS2> 16x2x4     11 <4,8,2,2>   8x8x4    12 <4,8,1,1>   8x4x4
    13 <2,32,4,2> fused 2x2x2 max-pool, 32x4x4
    14 k = 1, W >= 24, 32x1x4  15 k = 1, W 12..23, 16x2x4  16 k = 1, W < 12, 8x4x4       (<32,XB,1,2>)
    17 stem 5^3 + pool         18 stem, cout <= 32         19 stem, cout 33..64          (conv3d_stem5_kernel, 32x4x4)

Conditions of the table (each holds for at least one case of every variant; `LEAD` below names one case per variant that holds all of
them at once):
  ragged   >= 2 tiles along z, y and x, and D % tile_z, H % tile_y (where tile_y > 1), W % tile_x all non-zero
  chunks   odd cin, cin % cc != 0, >= 2 chunks of cc input channels (not the stem: its one input channel has no chunks)
  couts    cout % (32 * ncb) != 0, and >= 2 cout tiles where the variant admits them (not the cout <= 32 variants and the stem)
  batch    batch 2
  cost     2 * k^3 * B * cin * cout * D * H * W <= 2.5 GFLOP

Error bound of the random-data tests, per element (derived, not fitted):
    |got - y| <= 2 * n_acc * 2^-24 * C + 2^-24 * |y|,     C = sum |w| |x| (an fp64 conv of the absolute values)
    n_acc = 27 * cin + 3 (k = 3), cin + 3 (k = 1), 128 (stem: 125 taps + 3)
one rounding per product entering the fp32 accumulator, plus the K-split join and two epilogue operations; the factor 2 is the C3 that
tests/f16x2_contract.py allows for an accumulate that truncates.  The last term is the rounding of the stored result.

Largest measured |got - y| / bound per variant: not measured yet - tests/test_gpu_direct_conv.py prints them (pytest -s), one line per
case and the worst per variant at the end of the module.
"""
import collections

import torch
import torch.nn.functional as F

F64 = torch.float64
CAP_FLOP = 2.5e9
C3 = 2.0                      # tests/f16x2_contract.py: the allowance for a truncating accumulate

Case = collections.namedtuple("Case", "variant batch cin cout D H W k pool")


def _c(variant, batch, cin, cout, D, H, W, k=3, pool=False):
    return Case(variant, batch, cin, cout, D, H, W, k, pool)


# one case per variant that is ragged on every axis, has an odd cin with a partial last chunk, a half-empty last cout tile and batch 2
LEAD = (
    _c(0, 2, 7, 20, 6, 7, 61),
    _c(1, 2, 7, 20, 6, 7, 45),
    _c(2, 2, 7, 20, 6, 11, 21),
    _c(3, 2, 3, 70, 33, 34, 61),          # (vox / 512) * 2 = 534 >= 512 workgroups of the 32x4x4 tile
    _c(4, 2, 17, 70, 18, 15, 61),         # (vox / 256) * 2 = 256: the lower edge of the K-split 32x2x4 tile
    _c(5, 2, 17, 70, 6, 13, 61),
    _c(6, 2, 3, 70, 18, 15, 61),          # the same map with cin < 16: no K split
    _c(7, 2, 7, 70, 6, 5, 61),
    _c(8, 2, 5, 70, 34, 43, 45),          # (vox / 256) * 2 = 1026 >= 1024
    _c(9, 2, 7, 40, 6, 7, 45),
    _c(10, 2, 17, 40, 6, 7, 45),
    _c(11, 2, 5, 70, 38, 42, 21),         # (vox / 256) * 2 = 522 >= 512
    _c(12, 2, 7, 40, 6, 7, 21),
    _c(13, 2, 3, 70, 7, 9, 61, pool=True),
    _c(14, 2, 33, 70, 6, 5, 61, k=1),
    _c(15, 2, 33, 70, 6, 5, 21, k=1),
    _c(16, 2, 33, 70, 6, 7, 11, k=1),
    _c(17, 2, 1, 20, 7, 9, 45, k=5, pool=True),
    _c(18, 2, 1, 20, 6, 7, 45, k=5),
    _c(19, 2, 1, 48, 6, 7, 45, k=5),
)

# further edges: full chunks and full cout tiles next to the partial ones, one tile, batch 1, the other side of a threshold
MORE = (
    _c(0, 1, 8, 32, 4, 4, 32),            # exactly one full tile, full chunks, a full cout block
    _c(3, 1, 4, 70, 36, 61, 60),          # two full chunks, batch 1
    _c(4, 1, 16, 70, 19, 29, 60),         # two full chunks for each K-split half, batch 1
    _c(5, 1, 19, 100, 10, 14, 61),        # cout tiles 64 + 36
    _c(10, 1, 16, 64, 5, 6, 44),          # full chunks, full cout blocks
    _c(12, 1, 17, 33, 3, 5, 7),           # a map smaller than one tile on every axis
    _c(13, 1, 5, 33, 5, 7, 25, pool=True),
    _c(14, 1, 64, 35, 3, 2, 24, k=1),     # the RPN head's 35 anchors; W at the threshold
    _c(15, 1, 32, 64, 2, 3, 12, k=1),     # W at the threshold
    _c(16, 1, 7, 6, 3, 3, 3, k=1),
    _c(17, 1, 1, 32, 5, 6, 33, k=5, pool=True),
    _c(18, 1, 1, 32, 5, 6, 33, k=5),
    _c(19, 1, 1, 33, 5, 6, 33, k=5),
    _c(19, 1, 1, 64, 3, 5, 31, k=5),
)

CASES = LEAD + MORE

# gradient cases (batch, cin, cout, D, H, W, k) for conv3d_wgrad / conv3d_bias_grad, chosen from conv3d_wgrad.hip's own edges: its voxel
# tile is 16 x 4 x 2; it loads 16-byte quads of four x, which cross rows when W % 4 != 0, start before the tensor's first element at the
# first halo row (the shift path) and run past its end; 32-channel blocks of cin and cout; split-K over min(tiles, 1024 / blocks) slots
WGRAD_CASES = (
    (1, 4, 5, 2, 4, 16, 3),               # exactly one tile: the split count is capped at 1
    (3, 33, 70, 1, 3, 3, 3),              # D = 1, H < 4, W = 3, batch 3, cin and cout one past a 32-block / 6 past two
    (2, 7, 33, 3, 5, 6, 3),               # W = 6 (W % 4 = 2)
    (1, 33, 7, 2, 2, 9, 3),               # W = 9 (W % 4 = 1)
    (2, 5, 6, 5, 9, 19, 3),               # W % 4 = 3, two x tiles
    (1, 70, 33, 3, 4, 8, 3),              # W % 4 = 0, three cin blocks
    (2, 3, 40, 11, 22, 40, 3),            # 216 tiles
    (3, 33, 70, 3, 5, 7, 1),              # k = 1: four voxel groups per split slot
    (1, 5, 6, 2, 4, 18, 1),
    (2, 1, 20, 5, 6, 19, 5),              # k = 5 stem
    (1, 1, 48, 3, 7, 33, 5),
)

# conv3d_stem5_dgrad (batch, channels, D, H, W): ragged against its 32 x 16 x 8 tile, two tiles along every axis
STEM_DGRAD_CASES = ((2, 20, 9, 17, 33), (2, 48, 9, 17, 33))


def case_id(c):
    return "v%d-b%d-%dto%d-%dx%dx%d-k%d%s" % (c.variant, c.batch, c.cin, c.cout, c.D, c.H, c.W, c.k, "-pool" if c.pool else "")


def flop(c):
    return 2.0 * c.k ** 3 * c.batch * c.cin * c.cout * c.D * c.H * c.W


def n_acc(c):
    """roundings that enter one output element (the module docstring)"""
    return 128 if c.k == 5 else c.k ** 3 * c.cin + 3


def bound(c, y, cabs):
    """the per-element error bound; y = the fp64 result, cabs = the fp64 conv of the absolute values"""
    return C3 * n_acc(c) * 2.0 ** -24 * cabs + 2.0 ** -24 * y.abs()


def integers(shape, lo, hi, gen):
    """integer-valued fp32 in [lo, hi]"""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


def conv64(x, w, k):
    return F.conv3d(x.to(F64), w.to(F64), padding=k // 2)


def dgrad64(gy, w, k):
    """backward-data of the stride-1 'same' conv with weight w [cout_w, cin_w, k, k, k]: gy [B, cout_w, ...] -> [B, cin_w, ...]"""
    shape = (gy.shape[0], w.shape[1]) + tuple(gy.shape[2:])
    return torch.nn.grad.conv3d_input(shape, w.to(F64), gy.to(F64), padding=k // 2)


def exact_condition(*abs_terms):
    """every fp32 summation order of integer products is exact when sum |w| |x| stays below 2^24: the largest such sum"""
    return max(float(t.max()) for t in abs_terms)


def pool_gather(y, argmax):
    """y [B, C, D, H, W] at the positions a 2x2x2 pool's arg-max (q = dz * 4 + dy * 2 + dx inside the window) names"""
    B, Cc, OD, OH, OW = argmax.shape
    q = argmax.long()
    oz, oy, ox = torch.meshgrid(torch.arange(OD), torch.arange(OH), torch.arange(OW), indexing="ij")
    z, yy, x = 2 * oz + (q >> 2), 2 * oy + ((q >> 1) & 1), 2 * ox + (q & 1)
    lin = (z * y.shape[3] + yy) * y.shape[4] + x
    return y.reshape(B, Cc, -1).gather(2, lin.reshape(B, Cc, -1)).reshape(argmax.shape)
