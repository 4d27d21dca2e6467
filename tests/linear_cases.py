"""The case table of the forward linear GEMMs of csrc/fc_gemm.hip, their operands, fp64 reference, per-element error bound and a NumPy
emulation.  No tests live here: tests/test_linear_cases_host.py proves on the CPU that the table reaches every instance under the conditions
below (against m3d_linear_plan, the library's own host query), that the integer operands are exact and that every seeded defect is caught;
tests/test_gpu_linear_forward.py runs the table on the GPU.

Instances (the kernel instantiation a case must run; m3d_linear_plan's tile and slice counts name it)
  f32.full   fc_gemm_kernel, 128 x 128 tiles: every row tile on the full-tile path (M % 128 == 0 or > 64)
  f32.tail1  the same kernel with a last row tile of ONE 32-row block (M % 128 in 1..32): the tail path, its own slice count slices_tail
  f32.tail2  ... of TWO 32-row blocks (M % 128 in 33..64)
  x3.128     fc_x3_gemm_kernel<2>      bf16x3, 128 x 128 tiles on the packed planes
  x3.256     fc_x3_gemm_kernel<4>      bf16x3, 256 x 128
  x3.w32     fc_x3b_gemm_kernel<0>     bf16x3, 256 x 256, both operands cut in the kernel
  f16.128    fc_x3_gemm_kernel<2,0,1>  f16x2, 128 x 128
  f16.256    fc_x3_gemm_kernel<4,0,1>  f16x2, 256 x 128
  f16.big    fc_x3b_gemm_kernel<1>     f16x2, 256 x 256 (from 384 rows and 256 columns on)
A case is reached by the release library as it plans the shape (knobs == ()), or by the tuning library with the options in `knobs`.  At
these sizes the release planners never choose the 128-row tile of the split kernels, a slice of one chunk, or different slice counts for the
full and the tail tiles of the fp32 kernel: those come from tune_fc_x3_rows, tune_fc_slices and tune_fc_slices_tail.

K is cut into chunks of 32; slice s of n covers chunks [s * chunks / n, (s + 1) * chunks / n).  With slices == 1 the GEMM's own epilogue
adds the bias, applies the ReLU and stores; otherwise the slices' partial sums go to the workspace and fc_reduce_kernel adds them in slice
order, then bias and ReLU, once.

Integer operands (integer_operands): every value is an integer, so every product and every partial sum of any order is an integer, and
sum_k |x_k w_k| < 2^24 for every output (the host test computes it), so fp32 holds each of them exactly: the result must EQUAL the fp64
reference.  Base elements are integers in [-2, 2].  For the split kernels every 32-wide chunk of every row of x and of w holds probes at fixed
positions in the chunk, whose cut fills the lower planes, paired so that only products the kernel keeps are non-zero:
  bf16x3 (cut by truncation into h, m, l of 8 significand bits; kept hh hm mh hl lh mm, dropped ml lm ll)
    position 5   x = +-(2^18 + 2^9 + 1)  (h, m, l = 2^18, 2^9, 1)    w = +-1                   three planes against one
    position 14  x = +-(2^9 + 1)         (h, m = 2^9, 1)             w = +-(2^9 + 1)           two against two
    position 27  x = +-1                                             w = +-(2^18 + 2^9 + 1)    one against three
    The bit groups are nine positions apart: under truncation and under round-to-nearest-even alike the top eight bits are the first
    group alone (the rest is below half an ulp), so the planes do not depend on the rounding mode of the cut.
  f16x2 (scale by the power of two of f16_scale_of, h = fp16(v), l = fp16(v - h), 11 significand bits; kept hh hl lh, dropped ll)
    position 5   x = +-(2^13 + c), c in 1..3  (h, l = 2^13, c)       w in +-1, +-2             two planes against one
    position 27  x in +-1, +-2                                       w = +-(2^13 + c)          one against two
    max |x| = max |w| = 2^13 + 3, so the scale of an exact bound (and of a swept one) is 2, of a bound loose by 2^8 it is 2^-7: l = c * 2 or
    c * 2^-7 is a normal fp16 number either way, and the cut is exact under all three.
A probe product is about 2^18 (bf16x3) or 2^14 (f16x2), so one output can afford 16 resp. 256 chunks with non-zero probe products:
where a case has more chunks, w's probe elements of column n are non-zero only in the chunks c with c % P == n % P
(P = ceil(chunks / 16) resp. / 256; x keeps its probes everywhere, and every chunk is live for some column).

Error bound of the random-data tests, per element (derived, not fitted); S = sum_k |x_k w_k| + |bias|, y the fp64 result, u = 2^-24:
  fp32    gamma_n S + u |y|, n = K + 64, gamma_n = n u / (1 - n u): tests/linear_backward_reference.py (Higham 3.1: any summation order; K
          fused multiply-adds, at most 64 slices by the planners' contract - not read from the plan under test - whose 63 additions and the
          bias add are n's last 64).
  bf16x3  (1 + 2^-6) gamma_n S + (2^-20 + 2^-28) S + u |y|.  The cut is exact (h + m + l = x), so the kept products differ from x w by the
          dropped ones only.  Truncation to 8 bits: |x - h| < 2^-7 |x|, so |m| < 2^-7 |x|, and |l| = |(x - h) - m| < 2^-7 |x - h| <
          2^-14 |x|; hence |m_x l_w| + |l_x m_w| + |l_x l_w| < (2^-21 + 2^-21 + 2^-28) |x w|.  The kept products' magnitudes sum to at most
          (1 + 2^-7)^2 S < (1 + 2^-6) S, which is what the accumulation rounds: 6 K / 16 MFMA accumulations, each below 2 u of the running
          sum even if the MFMA truncates (tests/f16x2_contract.py: c3 = 2), are 0.75 K u < K u, and the slices and the bias as above.
  f16x2   f16x2_contract.bound("fc", ...) with A = the x bound given (or max |x|), B = max |w|, as test_split_linear_f16_meets_the_contract.
Where S == 0 the output must be exactly the bias (or its ReLU).

Largest measured |got - y| / bound per instance (MI355X; tests/test_gpu_linear_forward.py prints them with pytest -s) are recorded in that
module's docstring."""
import collections

import numpy as np

import f16x2_contract as F16C
import linear_backward_reference as R

CAP_MAC = 0.5e9                   # multiply-adds per case (the cap of wino_conv_cases.CAP_FLOP)
BK = 32
SENTINEL = -98765.0               # fills the buffer around and under `out`; no integer case produces it
KINDS = {"f32": 0, "x3": 1, "x3.w32": 2, "f16": 3}
TILE = {"f32.full": (128, 128), "f32.tail1": (128, 128), "f32.tail2": (128, 128), "x3.128": (128, 128), "x3.256": (256, 128),
        "x3.w32": (256, 256), "f16.128": (128, 128), "f16.256": (256, 128), "f16.big": (256, 256)}
INSTANCES = tuple(TILE)
LIVE = {"x3": 16, "f16": 256}    # chunks with non-zero probe products one output can afford

Case = collections.namedtuple("Case", "inst M N K slices slices_tail knobs")


def _c(inst, M, N, K, slices, slices_tail=None, **knobs):
    if slices_tail is None:                       # m3d_linear_plan: 1 where the fp32 kernel has no tail tile, `slices` for the other kernels
        slices_tail = 1 if inst == "f32.full" else slices
    return Case(inst, M, N, K, slices, slices_tail, tuple(sorted(knobs.items())))


ROWS128 = dict(tune_fc_x3_rows=128)
CASES = (
    # ---- fp32, every row tile on the full path
    _c("f32.full", 256, 128, 32, 1),                                  # exact multiples, K = 32: one chunk
    _c("f32.full", 200, 130, 100, 2),                                 # K % 32 = 4: slices of two chunks, the last chunk one quad
    _c("f32.full", 223, 161, 132, 3, tune_fc_slices=3),               # 5 chunks as 1, 2, 2, the last partial; 95 rows in the last tile
    _c("f32.full", 193, 200, 256, 3),                                 # 8 chunks as 2, 3, 3; 65 rows in the last tile
    _c("f32.full", 384, 256, 64, 1),                                  # exact multiples, 3 x 2 tiles
    _c("f32.full", 205, 72, 96, 1),                                   # ragged both ways with the GEMM's own stores
    # ---- fp32, last row tile one 32-row block
    _c("f32.tail1", 129, 130, 160, 2, 3, tune_fc_slices=2, tune_fc_slices_tail=3),      # one valid row; tail 1, 2, 2, full 2, 3
    _c("f32.tail1", 1, 128, 32, 1),                                   # no full tile, one row, one chunk
    _c("f32.tail1", 31, 200, 64, 1),                                  # no full tile, 31 rows
    _c("f32.tail1", 160, 72, 1024, 9),                                # a whole block of 32 rows; one ragged column tile
    _c("f32.tail1", 130, 256, 64, 1),                                 # slices == 1 with a full tile in front
    _c("f32.tail1", 129, 128, 128, 2, 1, tune_fc_slices=2, tune_fc_slices_tail=1),      # full tiles reduced, tail stored directly
    _c("f32.tail1", 150, 136, 100, 1, 2, tune_fc_slices=1, tune_fc_slices_tail=2),      # full tiles direct, tail reduced: 4 chunks as 2, 2
    _c("f32.tail1", 278, 161, 132, 2, 5, tune_fc_slices=2, tune_fc_slices_tail=5),      # two full row tiles; tail slices of one chunk each
    # ---- fp32, last row tile two 32-row blocks
    _c("f32.tail2", 33, 130, 160, 2),                                 # no full tile, 33 rows
    _c("f32.tail2", 191, 128, 32, 1),                                 # 63 rows in the tail
    _c("f32.tail2", 192, 256, 256, 3),                                # 64 rows: both blocks whole
    _c("f32.tail2", 170, 161, 132, 3, 2, tune_fc_slices=3, tune_fc_slices_tail=2),      # full 1, 2, 2; tail 2, 3
    _c("f32.tail2", 161, 130, 96, 1, 3, tune_fc_slices=1, tune_fc_slices_tail=3),       # full direct, tail three slices of one chunk
    _c("f32.tail2", 40, 72, 36, 1),                                   # no full tile, K = 36: one whole chunk and one quad
    _c("f32.tail2", 180, 128, 128, 2, 1, tune_fc_slices=2, tune_fc_slices_tail=1),      # full tiles reduced, tail stored directly
    # ---- bf16x3, 128 x 128
    _c("x3.128", 129, 130, 160, 3, tune_fc_slices=3, **ROWS128),      # one valid row; 1, 2, 2; 4 tiles x 3
    _c("x3.128", 256, 256, 64, 1, **ROWS128),                         # exact multiples
    _c("x3.128", 159, 72, 512, 3, **ROWS128),                         # 16 chunks as 5, 5, 6; 31 rows
    _c("x3.128", 161, 200, 96, 1, **ROWS128),                         # 33 rows
    # ---- bf16x3, 256 x 128
    _c("x3.256", 257, 130, 160, 3, tune_fc_slices=3, tune_fc_x3_rows=256),        # the slice count is only forced with the tile height
    _c("x3.256", 512, 256, 64, 1),
    _c("x3.256", 287, 72, 512, 3),
    _c("x3.256", 289, 200, 96, 1),
    # ---- bf16x3, 256 x 256 on the fp32 weight
    _c("x3.w32", 257, 258, 160, 3, tune_fc_slices=3),
    _c("x3.w32", 512, 512, 64, 1),
    _c("x3.w32", 287, 300, 512, 3),
    _c("x3.w32", 289, 72, 96, 1),                                     # fewer weight rows than a half tile: the clamped loads
    # ---- f16x2, 128 x 128
    _c("f16.128", 129, 130, 160, 3, tune_fc_slices=3, **ROWS128),
    _c("f16.128", 256, 256, 64, 1, **ROWS128),
    _c("f16.128", 159, 72, 512, 3, **ROWS128),
    _c("f16.128", 161, 200, 96, 1, **ROWS128),
    # ---- f16x2, 256 x 128
    _c("f16.256", 257, 130, 160, 3, tune_fc_slices=3, tune_fc_x3_rows=256),
    _c("f16.256", 512, 128, 64, 1),                                   # 384 rows or more but fewer than 256 columns
    _c("f16.256", 287, 72, 512, 3),
    _c("f16.256", 289, 200, 96, 1),
    _c("f16.256", 383, 256, 64, 1),                                   # one row below the 256 x 256 kernel's threshold
    _c("f16.256", 40, 136, 87808, 64),                                # fc1's reduction length at a few dozen rows
    # ---- f16x2, 256 x 256
    _c("f16.big", 513, 258, 160, 3, tune_fc_slices=3),                # one valid row in the third row tile; 6 tiles x 3
    _c("f16.big", 512, 512, 64, 1),
    _c("f16.big", 415, 300, 512, 3),                                  # 159 rows in the last tile
    _c("f16.big", 417, 264, 96, 1),                                   # 161 rows
    _c("f16.big", 384, 256, 64, 1),                                   # at the threshold
)


def case_id(c):
    k = "-".join("%s%d" % (n.replace("tune_fc_", ""), v) for n, v in c.knobs)
    return "%s-%dx%dx%d-s%d.%d%s" % (c.inst, c.M, c.N, c.K, c.slices, c.slices_tail, "-" + k if k else "")


def family(c):
    return c.inst.split(".")[0]


def kind_of(c):
    return KINDS["x3.w32"] if c.inst == "x3.w32" else KINDS[family(c)]


def expected_plan(c):
    """what m3d_linear_plan must answer for the case (inside the case's library context)"""
    tr, tc = TILE[c.inst]
    fm = -(-c.M // tr) - (1 if c.inst in ("f32.tail1", "f32.tail2") else 0)
    return dict(tile_rows=tr, tile_cols=tc, slices=c.slices, slices_tail=c.slices_tail, full_row_tiles=fm)


def chunks_of(c):
    return -(-c.K // BK)


def slice_ranges(chunks, n):
    return [(s * chunks // n, (s + 1) * chunks // n) for s in range(n)]


def row_groups(c):
    """[(first row, end row, slices)]: the rows of the full tiles and, for the fp32 kernel, those of the ragged last tile on its tail path"""
    if family(c) == "f32" and c.inst != "f32.full":
        full = (c.M - 1) // 128 * 128
        return ([(0, full, c.slices)] if full else []) + [(full, c.M, c.slices_tail)]
    return [(0, c.M, c.slices)]


def slice_lengths(c):
    return [[c1 - c0 for c0, c1 in slice_ranges(chunks_of(c), n)] for _, _, n in row_groups(c)]


def units(c):
    """workgroups with work per group of row_groups (tiles x slices)"""
    tr, tc = TILE[c.inst]
    nt = -(-c.N // tc)
    return [-(-(r1 - r0) // tr) * nt * n for r0, r1, n in row_groups(c)]


# ------------------------------------------------------------------ the cuts
def cut_bf16(a):
    """h, m, l (fp32 arrays) as the kernels cut an fp32 array: the top 16 bits, the top 16 bits of the rest, the rest (truncated alike)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    top = lambda v: (np.ascontiguousarray(v).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    h = top(a)
    r1 = a - h
    m = top(r1)
    return [h, m, top(r1 - m)]


def cut_f16(a, bound):
    """(h, l) in SCALED units (fp32 arrays holding fp16 values) and (s, 1 / s) of f16_scale_of(bound)"""
    s, inv = F16C.scale_of(bound)
    v = np.ascontiguousarray(a, dtype=np.float32) * np.float32(s)
    h = v.astype(np.float16)
    l = (v - h.astype(np.float32)).astype(np.float16)
    return [h.astype(np.float32), l.astype(np.float32)], (s, inv)


def planes(c, a, bound=None):
    """the planes of operand `a` in its own units, fp64 (they must sum to `a` where the cut is exact)"""
    if family(c) == "x3":
        return [p.astype(np.float64) for p in cut_bf16(a)]
    p, (s, _) = cut_f16(a, float(np.abs(a).max()) if bound is None else bound)
    return [q.astype(np.float64) / s for q in p]


def cut_is_exact(c, x, w, x_bound=None):
    """the integer operands stay exact under the scale of `x_bound`: the planes sum to the operands and no dropped product is non-zero
    (with sum |x w| < 2^24 this is the whole condition; tests/test_linear_cases_host.py holds the emulation against it)"""
    if family(c) == "f32":
        return True
    px, pw = planes(c, x, x_bound), planes(c, w)
    return (np.array_equal(sum(px), x.astype(np.float64)) and np.array_equal(sum(pw), w.astype(np.float64))
            and not any((np.abs(px[ia]) @ np.abs(pw[ib]).T).any() for ia, ib in DROPPED[family(c)]))


# products of one k16 step in the kernels' order (index of the x plane, of the w plane), small terms first
PRODUCTS = {"f32": [(0, 0)], "x3": [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], "f16": [(1, 0), (0, 1), (0, 0)]}
DROPPED = {"x3": [(1, 2), (2, 1), (2, 2)], "f16": [(1, 1)]}

DEFECTS = ("short_slice", "bias_per_slice", "relu_per_slice", "row_mask_short", "row_mask_long", "col_mask_short", "col_mask_long",
           "tail_full_slices", "drop_low_product", "dup_product", "col_block_neighbour")


def defect_applies(c, d):
    tr, tc = TILE[c.inst]
    if d == "short_slice":
        return any(n <= 2 for ls in slice_lengths(c) for n in ls)
    if d in ("bias_per_slice", "relu_per_slice"):
        return any(n > 1 for _, _, n in row_groups(c))
    if d == "row_mask_long":                      # a lane for row M exists, and the store is the GEMM's own
        return c.M % 32 != 0 and row_groups(c)[-1][2] == 1
    if d == "col_mask_long":
        return c.N % 32 != 0 and row_groups(c)[-1][2] == 1
    if d == "tail_full_slices":
        return len(row_groups(c)) == 2 and c.slices != c.slices_tail
    if d in ("drop_low_product", "dup_product"):
        return family(c) != "f32"
    if d == "col_block_neighbour":
        return c.N > tc
    return True


def emulate(c, x, w, bias=None, relu=False, dtype=np.float32, x_bound=None, defect=None):
    """The launch in NumPy at `dtype`: the operands cut into planes as the kernel cuts them, per K slice the chunks in order and per chunk the
    kept products in the kernels' order, each slice's partial sum on its own; slices == 1: bias and ReLU in the GEMM's epilogue, else the
    reduce kernel's sum in slice order, then bias and ReLU; stores through the row and column masks of each tile.  Returns the flat buffer
    the GPU test hands the kernel: (M + 1) * N + 1 elements of SENTINEL with out[M, N] at its start.  A value that is read before anything
    wrote it is NaN.  defect: one of DEFECTS, a seeded fault."""
    assert defect is None or defect_applies(c, defect), (c, defect)
    fam = family(c)
    M, N, K = c.M, c.N, c.K
    tr, tc = TILE[c.inst]
    x, w = np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(w, dtype=np.float32)
    unscale = (1.0, 1.0)
    if fam == "f32":
        px, pw = [x], [w]
    elif fam == "x3":
        px, pw = cut_bf16(x), cut_bf16(w)
    else:
        px, (_, ix) = cut_f16(x, float(np.abs(x).max()) if x_bound is None else x_bound)
        pw, (_, iw) = cut_f16(w, float(np.abs(w).max()))
        unscale = (ix, iw)
    px, pw = [p.astype(dtype) for p in px], [p.astype(dtype) for p in pw]
    prods = list(PRODUCTS[fam])
    if defect == "drop_low_product":
        prods = prods[1:]
    if defect == "dup_product":
        prods[1] = prods[0]
    b = None if bias is None else np.asarray(bias, dtype=dtype)
    chunks = chunks_of(c)
    nan = dtype(np.nan)
    out = np.full((M + 1) * N + 1, dtype(SENTINEL), dtype=dtype)
    o2 = out[:M * N].reshape(M, N)
    groups = row_groups(c)

    def epilogue(v):
        if b is not None:
            v = v + b[None, :]
        return np.maximum(v, dtype(0)) if relu else v

    for gi, (r0, r1, nsl) in enumerate(groups):
        parts = []
        for c0, c1 in slice_ranges(chunks, nsl):
            if defect == "short_slice" and c1 - c0 <= 2:
                c1 -= 1
            acc = np.zeros((r1 - r0, N), dtype=dtype)
            for ch in range(c0, c1):
                ks = slice(ch * BK, min(K, (ch + 1) * BK))
                for ia, ib in prods:
                    acc = acc + px[ia][r0:r1, ks] @ pw[ib][:, ks].T
            if fam == "f16":
                acc = (acc * dtype(unscale[0])) * dtype(unscale[1])
            parts.append(acc)
        if nsl == 1:
            res = epilogue(parts[0])
        else:
            if defect == "bias_per_slice" and b is not None:
                parts = [p + b[None, :] for p in parts]
            if defect == "relu_per_slice" and relu:
                parts = [np.maximum(p, dtype(0)) for p in parts]
            ns = nsl
            if defect == "tail_full_slices" and gi == 1:
                ns = c.slices
            if ns == 1:                           # the reduce kernel skips rows of one slice: nothing stores these
                continue
            v = parts[0]
            for s in range(1, ns):
                v = v + (parts[s] if s < nsl else nan)
            res = v + b[None, :] if (b is not None and defect != "bias_per_slice") else v
            res = np.maximum(res, dtype(0)) if relu else res
        o2[r0:r1] = res
    direct_last = groups[-1][2] == 1
    if defect == "row_mask_short":
        o2[M - 1] = dtype(SENTINEL) if direct_last else nan
    if defect == "row_mask_long":                 # the lane of row M holds row M - 1's data (clamped loads)
        out[M * N:(M + 1) * N] = o2[M - 1]
    if defect == "col_mask_short":
        o2[:, N - 1] = dtype(SENTINEL) if direct_last else nan
    if defect == "col_mask_long":                 # column N of row m is element 0 of row m + 1; the last row's lands behind `out`
        out[M * N] = o2[M - 1, N - 1]
    if defect == "col_block_neighbour":           # row tile 0: the first 32 columns of column tile 0 land in column tile 1
        rows = slice(0, min(tr, M))
        width = min(32, N - tc)
        o2[rows, tc:tc + width] = o2[rows, :width]
        o2[rows, :32] = dtype(SENTINEL) if groups[0][2] == 1 else nan
    return out


def expected_buffer(ref, dtype=np.float32):
    M, N = ref.shape
    out = np.full((M + 1) * N + 1, dtype(SENTINEL), dtype=dtype)
    out[:M * N] = np.asarray(ref, dtype=dtype).reshape(-1)
    return out


# ------------------------------------------------------------------ operands
X3_THREE = float(2 ** 18 + 2 ** 9 + 1)
X3_TWO = float(2 ** 9 + 1)
F16_TWO = float(2 ** 13)
POS = {"x3": (5, 14, 27), "f16": (5, 27)}


def live_period(c):
    return -(-chunks_of(c) // LIVE[family(c)]) if family(c) != "f32" else 1


def _seed(c, extra=0):
    return (c.M * 1000003 + c.N * 1009 + c.K * 11 + KINDS[family(c)] + 17 * extra) % (2 ** 31)


def integer_operands(c):
    """x [M, K], w [N, K], bias [N] (fp32, integer-valued; the module docstring).  Cases of one family and shape share them."""
    rng = np.random.RandomState(_seed(c))
    M, N, K = c.M, c.N, c.K
    x = rng.randint(-2, 3, (M, K)).astype(np.float32)
    w = rng.randint(-2, 3, (N, K)).astype(np.float32)
    x[0, 0], x[-1, -1], w[0, 0], w[-1, -1] = 2.0, -2.0, 1.0, 2.0        # the corners carry data
    fam = family(c)
    if fam != "f32":
        chunks = K // BK
        sign = lambda shape: (1 - 2 * rng.randint(0, 2, shape)).astype(np.float32)
        live = (np.arange(chunks)[None, :] % live_period(c) == np.arange(N)[:, None] % live_period(c)).astype(np.float32)   # [N, chunks]
        xv, wv = x.reshape(M, chunks, BK), w.reshape(N, chunks, BK)
        if fam == "x3":
            p3, p2, p1 = POS["x3"]
            xv[:, :, p3] = sign((M, chunks)) * np.float32(X3_THREE)
            wv[:, :, p3] = sign((N, chunks)) * live
            xv[:, :, p2] = sign((M, chunks)) * np.float32(X3_TWO)
            wv[:, :, p2] = sign((N, chunks)) * np.float32(X3_TWO) * live
            xv[:, :, p1] = sign((M, chunks))
            wv[:, :, p1] = sign((N, chunks)) * np.float32(X3_THREE) * live
        else:
            p2, p1 = POS["f16"]
            xv[:, :, p2] = sign((M, chunks)) * (np.float32(F16_TWO) + rng.randint(1, 4, (M, chunks)).astype(np.float32))
            wv[:, :, p2] = sign((N, chunks)) * rng.randint(1, 3, (N, chunks)).astype(np.float32) * live
            xv[:, :, p1] = sign((M, chunks)) * rng.randint(1, 3, (M, chunks)).astype(np.float32)
            wv[:, :, p1] = sign((N, chunks)) * (np.float32(F16_TWO) + rng.randint(1, 4, (N, chunks)).astype(np.float32)) * live
            x[0, p2], w[0, p1] = F16_TWO + 3, F16_TWO + 3                # max |x| = max |w| = 2^13 + 3 whatever the draw
            w[0, p2] = 1.0 if w[0, p2] == 0 else w[0, p2]
    bias = rng.randint(-8, 9, (N,)).astype(np.float32)
    return x, w, bias


def random_operands(c):
    """x rows at per-row powers of two over 2^20, every seventh row zero, ReLU-like for the split kernels; w ~ 0.2 N(0, 1) with per-row
    powers of two over 2^4 and one zero row; bias ~ N(0, 1)"""
    rng = np.random.RandomState(_seed(c, 1))
    M, N, K = c.M, c.N, c.K
    x = rng.standard_normal((M, K)).astype(np.float32)
    if family(c) != "f32":
        x = np.maximum(x, np.float32(0))
    x *= (2.0 ** rng.randint(-10, 11, (M, 1))).astype(np.float32)
    x[3::7] = 0
    w = (rng.standard_normal((N, K)) * 0.2).astype(np.float32) * (2.0 ** rng.randint(-2, 3, (N, 1))).astype(np.float32)
    w[N // 2] = 0
    return x, w, rng.standard_normal((N,)).astype(np.float32)


# ------------------------------------------------------------------ reference and bound
def reference(x, w, bias=None, relu=False):
    y = x.astype(np.float64) @ w.astype(np.float64).T
    if bias is not None:
        y = y + bias.astype(np.float64)[None, :]
    return np.maximum(y, 0.0) if relu else y


def magnitude(x, w, bias=None):
    S = np.abs(x.astype(np.float64)) @ np.abs(w.astype(np.float64)).T
    return S if bias is None else S + np.abs(bias.astype(np.float64))[None, :]


def bound(c, x, w, bias=None, relu=False, x_bound=None):
    """(y, E, S): the fp64 reference, the per-element error bound (the module docstring) and S = sum |x w| (without the bias)"""
    import torch
    fam = family(c)
    y = reference(x, w, bias, relu)
    S0 = magnitude(x, w)
    if fam == "f16":
        xt, wt = torch.from_numpy(x), torch.from_numpy(w)
        C, Sa, Sb, n = F16C.terms(F16C.linear_op, xt, wt)
        A = float(np.abs(x).max()) if x_bound is None else float(x_bound)
        E = F16C.bound("fc", c.K, C, Sa, Sb, n, A, float(np.abs(w).max()), torch.from_numpy(y)).numpy()
        return y, E, S0
    S = magnitude(x, w, bias)
    g = R.gamma(c.K + R.MAX_SLICES)
    if fam == "f32":
        return y, g * S + R.U * np.abs(y), S0
    return y, (1 + 2.0 ** -6) * g * S + (2.0 ** -20 + 2.0 ** -28) * S0 + R.U * np.abs(y), S0
