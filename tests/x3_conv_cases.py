"""The case table of the bf16x3 / f16x2 direct conv of csrc/conv3d_x3.hip (ops.X3Conv3d: out = conv3d(x - off, W or relu(W), padding 1), the
norm conv of the peak back-propagation), its operands, fp64 reference, per-element error bound and a NumPy emulation.  No tests live here:
tests/test_x3_conv_cases_host.py proves on the CPU, with the library's own host queries, that the table meets the conditions below, that the
integer operands are exact and that every seeded defect is caught on every case it applies to; tests/test_gpu_x3_conv.py runs the table on
the GPU.

A case is Case(form, mode, batch, cin, cout, D, H, W, ksplit, ws): form "x3" (bf16x3: both operands cut by truncation into h, m, l of 8
significand bits, six products kept) or "x3f" (f16x2: both operands scaled by a power of two and cut into two fp16 numbers, three products
kept); mode W_RELU (relu(W), an offset: the norm conv) or W_PLAIN (signed weights and inputs, no offset); ws False: the entry point without
a workspace (m3d_conv3d_x3_forward; the f16x2 form has no such entry point and gets a null workspace).  Both forms run the same shapes.

The launch.  A workgroup owns 64 output channels (two blocks of 32 rows) x a 16 x 4 x 4 (x, y, z) voxel tile: units = B x tiles x cout
tiles.  K = cin / 16 chunks of 27 taps.  Below 192 units the launch cuts K into `ksplit` 2 or 4 ranges of whole chunk PAIRS (range k of n
covers pairs [k pairs / n, (k + 1) pairs / n), pairs = ceil(chunks / 2)), each range writes its partial sums to the workspace and a reduce
kernel adds them in range order; never when B cout D H W % 4 != 0 (the reduce adds float4s) or without a workspace.  The ksplit of a
case is NOT restated from that rule: the host test reads it from m3d_conv3d_x3_workspace_bytes / (4 elems) and from
m3d_conv3d_x3_launch_units / units, which must agree with each other and with the table.  Inside a range the accumulators are added to
memory after every second chunk and after the last (a "flush"); the first flush of a range stores, later ones read, add and write back.

Conditions (each form meets every one with at least one case; the host test proves them):
  split      ksplit 1, 2 and 4; ksplit 2 with an odd pair count (cin 80 or 96: unequal ranges); ksplit 4 with cin 144 (9 chunks, 5 pairs:
             ranges of 2, 2, 2 and 3 chunks, the last ends on an even chunk); ksplit 4 with cin 128
  unsplit    1 chunk (cin 16); 2 chunks; 3 chunks (the last flush follows an even chunk); >= 5 chunks (the accumulators restart several
             times); a case unsplit only because it has >= 192 units, with units % 8 != 0 (surplus workgroups of the unit -> XCD map return
             early); a case with fewer than 8 units; a case unsplit only because elems % 4 != 0 (the same shape with W rounded to even
             splits); a case unsplit only because no workspace is passed (the same shape splits under _ws)
  tiles      >= 2 tiles with a non-zero remainder along x, y and z in one case; a single partial tile with W < 16, H < 4, D < 4; an odd W
  channels   cout % 64 in (0, 32] (the upper 32-row block of the last tile is empty); cout % 64 in (32, 64); cout < 32; >= 2 cout tiles
  batch      batch 2, once split and once unsplit (the partial-sum stride depends on B)
  cost       2 * 27 * B * cin * cout * D * H * W <= direct_conv_cases.CAP_FLOP

Reference: direct_conv_cases.conv64 on the operand the kernel cuts, a = fl32(x - off), and W or relu(W); zero padding of a (0 outside the
volume, not -off).  It is written on whole tensors and shares no index arithmetic with the kernel.

Integer operands (integer_operands; the recipe of linear_cases.integer_operands).  Every value is an integer and S = sum |a| |w| < 2^24 for
every output (the host test computes S in fp64), so fp32 holds every product and every partial sum of any order exactly: the result must
EQUAL the fp64 reference.  Base values: a in 0..2 (W_RELU; x = a + off with the integer off = -3 = min x, so fl32(x - off) = a) or -2..2
(W_PLAIN), w in -2..2 (W_RELU: the negative ones are cut by the relu).  In every 16-channel chunk fixed channels carry probes whose cut fills
the lower planes, paired channel by channel so that only products the kernel keeps are non-zero.  The input probe fills its channel at
every voxel; the weight probe sits at ONE tap per (output channel, chunk, probe) - the tap moves with all three, so every ring slot and
both register sets carry probes - and the channel's other taps are 0: one output receives at most one product per chunk and probe.
  bf16x3 (kept, as (w piece, a piece): hh hm mh mm hl lh; dropped ml lm ll)
    channel 3   a = +-(2^18 + 2^9 + 1)  (h, m, l = 2^18, 2^9, 1)   w = +-1                   three planes against one
    channel 8   a = +-(2^9 + 1)         (h, m = 2^9, 1)            w = +-(2^9 + 1)           two against two
    channel 13  a = +-1                                            w = +-(2^18 + 2^9 + 1)    one against three
    (signs only in W_PLAIN).  A probe product is about 2^18: 9 chunks x 3 probes = 27 of them, 7.1e6, plus the base values' 144 x 27 x 4.
  f16x2 (kept hh hl lh; dropped ll)
    channel 3   a = +-(2^13 + c), c in 1..3  (h, l = 2^13, c)      w in +-1, +-2             two planes against one
    channel 13  a in +-1, +-2                                      w = +-(2^13 + c)          one against two
    max a = max w = 2^13 + 3 in every case, so the scale of the exact in_max is 2 and that of an in_max loose by 2^8 is 2^-7: l = 2 c or
    2^-7 c is a normal fp16 number either way and the cut is exact under both (cut_is_exact; linear_cases.cut_bf16 / cut_f16 are the cuts).
Every kept (w piece, a piece) pair is non-zero for some output in every K range, in both chunk parities and in both 32-row blocks (the
host test checks it from the planes).

Emulation (emulate): the cut; per K range the chunks in order, per chunk the 27 taps in order, per tap the kept products in the kernel's
order (small ones first), each a [cout, 16] x [16, voxels] fp32 matrix product added to an fp32 accumulator; after every second chunk of the
range and after its last the accumulator (f16x2: times the two inverse scales) is stored to (first flush of the range) or added with
round-to-nearest to the range's sums, and restarts at 0; the ranges' sums are added in range order.  Memory nothing wrote is NaN, so a
read before a write shows.  `defect=` seeds one fault (DEFECTS); each must fail the integer comparison on every case defect_applies names:
  drop_w<i>_a<j>      one kept product dropped
  stale_tap           tap 7 of the last chunk takes the weights of tap 4 (a ring slot that was not refilled: three steps earlier)
  tap_z tap_y tap_x   tap 0 of the first chunk reads the input one voxel further along the axis
  pad_minus_off       voxels outside the volume read as 0 - off instead of 0                                  (W_RELU: off != 0)
  skip_first_chunk    the last K range starts one chunk late;  repeat_last_chunk: the first K range runs its last chunk twice
  first_flush_adds    the first flush of a range adds to what memory holds
  upper_block_past_cout  the upper 32-row block of the last cout tile is stored without the row check: rows >= cout land behind
                      the last item (the guard rows of `out`, or of the workspace when the launch splits)           (cout % 64 != 0)
  reduce_skips_last   the reduce kernel adds one range too few                                                       (ksplit > 1)
  colxy_swap          two lane groups of col_xy ((x 0..3, y 0) and (x 4..7, y 0) of every 16 x 2 patch) exchange their voxels between the
                      fragment read and the store                                                                       (W >= 8)

Error bound of the random-data tests, per element (derived, not fitted); S = sum |a| |w| (= y for the norm conv), y the fp64 result,
u = 2^-24, gamma_n = n u / (1 - n u):
  bf16x3  (1 + 2^-6) gamma_n S + (2^-20 + 2^-28) S + u |y|, the expression of linear_cases: the cut is exact (h + m + l = a), the kept
          products differ from a w by the dropped ones, below (2^-21 + 2^-21 + 2^-28) |a w|; the kept products' magnitudes sum to at most
          (1 + 2^-7)^2 S < (1 + 2^-6) S, which is what the accumulation rounds.  n counted from this kernel, per output element:
            products             0     a bf16 x bf16 product has 16 significand bits: exact in fp32
            MFMA accumulations   2 x 6 x 27 per chunk = 324 cin / 16: one v_mfma_f32_32x32x16_bf16 per tap and kept product adds 16 exact
                                 products to the accumulator; it may truncate, an error below 2 u of the running sum (c3 = 2 of
                                 tests/f16x2_contract.py)
            flushes              ceil(chunks / 2): one fp32 add each (the storing first flush of a range counted too: it only helps)
            reduce               ksplit - 1 adds
          n = 324 chunks + ceil(chunks / 2) + ksplit - 1   (n_roundings; 2921 at cin 144, gamma_n = 1.7e-4)
  f16x2   f16x2_contract.bound("x3f", cin, ...) with A = fl32(in_max - off) (or in_max), B = max relu(W) (or max |W|).  Its n_acc =
          81 cin / 16 + cin / 32 + 1 covers the split too: the flush adds and the reduce adds together are ceil(chunks / 2) - 1.
Where S == 0 the output must be exactly 0.0.

Random operands (random_operands).  W_RELU, as the PRM sees them: x = off + v with v >= 0 (a ReLU'd normal deviate times a power of two
that changes from one 3 x 3 x 3 block of voxels to the next over 2^-21 .. 1, so small N occur), the low columns along x held at the minimum
x = off (exact zeros of a, and of N where the whole support lies there), off = 0 for odd W and 0.37 for even W; relu(W) with per-row powers
of two and one row without a positive entry (N == 0 for that channel).  W_PLAIN: signed inputs, one zero weight row.

Largest measured |got - y| / bound (MI355X; tests/test_gpu_x3_conv.py prints them with pytest -s) per (form, ksplit):
  bf16x3  ksplit 1  0.0768    ksplit 2  0.0150    ksplit 4  0.0090
  f16x2   ksplit 1  0.0802    ksplit 2  0.0648    ksplit 4  0.0502
The emulation's own worst ratios (tests/test_x3_conv_cases_host.py prints them): bf16x3 0.0511, 0.0094, 0.0062; f16x2 0.0802, 0.0648, 0.0504.
These are measurements, not thresholds: the only threshold is ratio <= 1.  No integer case differed from its reference in any element."""
import collections
import functools

import numpy as np
import torch

import direct_conv_cases as DC
import f16x2_contract as F16C
import linear_cases as LC

F64 = torch.float64
W_PLAIN, W_RELU = 0, 1                    # ops.W_PLAIN, ops.W_RELU
TX, TY, TZ, TM = 16, 4, 4, 64             # the workgroup's voxel tile and cout tile (checked against m3d_conv3d_x3_launch_units)
CAP_FLOP = DC.CAP_FLOP
SENTINEL = -98765.0                       # fills the guard rows behind `out` and behind the workspace; no case produces it
GUARD_ROWS = 64                           # channel maps behind the last item: a cout tile's rows >= cout land there if stored unchecked
FORMS = ("x3", "x3f")
INT_OFF = -3.0                            # the integer offset of the W_RELU integer cases (= min x)

Case = collections.namedtuple("Case", "form mode batch cin cout D H W ksplit ws")

_R, _P = W_RELU, W_PLAIN
SHAPES = (
    # mode batch cin cout D  H  W  ksplit ws
    (_R, 1, 80, 40, 5, 6, 18, 2, True),       # 5 chunks, 3 pairs: ranges of 2 and 3 chunks; 2 ragged tiles along x, y and z; cout % 64 = 40
    (_R, 2, 96, 70, 3, 3, 12, 2, True),       # 6 chunks, 3 pairs: 2 and 4; batch 2 split; 2 cout tiles, the last with an empty upper block
    (_R, 1, 144, 24, 5, 5, 17, 4, True),      # 9 chunks, 5 pairs: 2, 2, 2, 3; cout < 32; odd W
    (_R, 1, 128, 96, 4, 4, 16, 4, True),      # 8 chunks, 4 pairs: 2 each; exactly one full voxel tile; cout % 64 = 32
    (_P, 1, 48, 64, 2, 7, 20, 2, True),       # 3 chunks, 2 pairs: 2 and 1; a full cout tile; signed
    (_P, 1, 112, 40, 3, 5, 9, 4, True),       # 7 chunks, 4 pairs: 2, 2, 2, 1; 2 units before the split; signed
    (_R, 1, 16, 40, 5, 6, 18, 1, True),       # 1 chunk
    (_P, 1, 32, 100, 3, 3, 7, 1, True),       # 2 chunks; a single partial tile, W < 16, H < 4, D < 4; 2 units; cout % 64 = 36; signed
    (_R, 1, 48, 34, 5, 5, 17, 1, True),       # 3 chunks, unsplit only because elems % 4 = 2 (W = 18 splits)
    (_R, 1, 80, 40, 5, 6, 18, 1, False),      # 5 chunks, unsplit only because no workspace is passed (the first shape)
    (_R, 2, 48, 8, 193, 5, 10, 1, True),      # 196 units (196 % 8 = 4), unsplit only because of them; batch 2 unsplit
)
CASES = tuple(Case(form, *s) for form in FORMS for s in SHAPES)


def case_id(c):
    return "%s-%s-b%d-%dto%d-%dx%dx%d-k%d%s" % (c.form, "relu" if c.mode == W_RELU else "plain", c.batch, c.cin, c.cout, c.D, c.H, c.W,
                                              c.ksplit, "" if c.ws else "-nows")


def cdiv(a, b):
    return (a + b - 1) // b


def chunks_of(c):
    return c.cin // 16


def pairs_of(c):
    return cdiv(chunks_of(c), 2)


def tiles(c):
    return cdiv(c.W, TX), cdiv(c.H, TY), cdiv(c.D, TZ)


def units(c):
    """workgroups before the K split"""
    tx, ty, tz = tiles(c)
    return c.batch * tx * ty * tz * cdiv(c.cout, TM)


def elems(c):
    return c.batch * c.cout * c.D * c.H * c.W


def flop(c):
    return 2.0 * 27 * c.batch * c.cin * c.cout * c.D * c.H * c.W


def queried_ksplit(L, c, **change):
    """(ksplit by m3d_conv3d_x3_workspace_bytes, ksplit by m3d_conv3d_x3_launch_units) of the case's shape under _ws, `change` replacing
    fields; L: the library with its restypes set (m3d._lib.lib())"""
    c = c._replace(**change)
    args = (c.batch, c.cin, c.cout, c.D, c.H, c.W)
    wsb, lu = int(L.m3d_conv3d_x3_workspace_bytes(*args)), int(L.m3d_conv3d_x3_launch_units(*args))
    assert wsb % (4 * elems(c)) == 0 and lu % units(c) == 0 and lu > 0, (c, wsb, lu)
    return (wsb // (4 * elems(c)) or 1), lu // units(c)


def k_ranges(c, ksplit=None):
    """[(first chunk, end chunk)] of the launch's K ranges (module docstring)"""
    n = c.ksplit if ksplit is None else ksplit
    ch, pr = chunks_of(c), pairs_of(c)
    return [(2 * (k * pr // n), min(ch, 2 * ((k + 1) * pr // n))) for k in range(n)]


# ------------------------------------------------------------------ the cut
# kept products of one tap in the kernel's order, as (w piece, a piece), small terms first; the dropped ones
PRODUCTS = {"x3": [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)], "x3f": [(1, 0), (0, 1), (0, 0)]}
DROPPED = {"x3": [(1, 2), (2, 1), (2, 2)], "x3f": [(1, 1)]}


def weights_of(c, w):
    """the weight operand: relu(W) in W_RELU mode"""
    return np.maximum(w, np.float32(0)) if c.mode == W_RELU else w


def operand_of(x, off):
    """a = fl32(x - off), the operand the kernel cuts"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return x if off is None else x - np.float32(off)


def a_bound(off, in_max):
    """A of the f16x2 cut: fl32(in_max - off), or in_max without an offset"""
    return float(np.float32(in_max) - np.float32(off)) if off is not None else float(np.float32(in_max))


def w_bound(wr):
    """B of the f16x2 cut: the largest positive entry of relu(W), the largest |W| in W_PLAIN mode"""
    return float(np.abs(wr).max())


def cut(c, a, wr, A=None):
    """(planes of a, planes of wr, (1 / s_a, 1 / s_w)): fp32 arrays in the units the kernel multiplies (f16x2: scaled)"""
    if c.form == "x3":
        return LC.cut_bf16(a), LC.cut_bf16(wr), (1.0, 1.0)
    pa, (_, ia) = LC.cut_f16(a, float(np.abs(a).max()) if A is None else A)
    pw, (_, iw) = LC.cut_f16(wr, w_bound(wr))
    return pa, pw, (ia, iw)


def planes64(c, a, wr, A=None):
    """the planes in the operands' own units, fp64 (they sum to the operands where the cut is exact)"""
    pa, pw, (ia, iw) = cut(c, a, wr, A)
    return [p.astype(np.float64) * ia for p in pa], [p.astype(np.float64) * iw for p in pw]


def cut_is_exact(c, a, wr, A=None):
    """the planes sum to the operands and no channel carries both planes of a dropped product (a channel of `a` meets only the same
    channel of `w`); with S < 2^24 this is the whole exactness condition - the host test holds the emulation against it"""
    pa, pw = planes64(c, a, wr, A)
    if not (np.array_equal(sum(pa), a.astype(np.float64)) and np.array_equal(sum(pw), wr.astype(np.float64))):
        return False
    for iw, ia in DROPPED[c.form]:
        if (np.abs(pa[ia]).sum((0, 2, 3, 4)) * np.abs(pw[iw]).sum((0, 2, 3, 4))).any():
            return False
    return True


# ------------------------------------------------------------------ the emulation
def _product_names(form):
    return tuple("drop_w%d_a%d" % p for p in PRODUCTS[form])


DEFECTS = _product_names("x3") + ("stale_tap", "tap_z", "tap_y", "tap_x", "pad_minus_off", "skip_first_chunk", "repeat_last_chunk",
                                  "first_flush_adds", "upper_block_past_cout", "reduce_skips_last", "colxy_swap")


def defect_applies(c, d, ksplit=None):
    n = c.ksplit if ksplit is None else ksplit
    if d.startswith("drop_"):
        return d in _product_names(c.form)
    if d == "pad_minus_off":
        return c.mode == W_RELU
    if d == "upper_block_past_cout":
        return c.cout % TM != 0
    if d == "reduce_skips_last":
        return n > 1
    if d == "colxy_swap":
        return c.W >= 8
    return True


Buffers = collections.namedtuple("Buffers", "out ws_guard")


def _buffers(c, out, split):
    """`out` [B, cout, D, H, W] followed by GUARD_ROWS channel maps of SENTINEL; the guard behind the workspace of a split launch"""
    dhw = c.D * c.H * c.W
    guard = np.full(GUARD_ROWS * dhw, np.float32(SENTINEL), dtype=np.float32)
    return Buffers(np.concatenate([np.asarray(out, dtype=np.float32).reshape(-1), guard]), guard.copy() if split else None)


def expected(c, ref, ksplit=None):
    """the buffers a correct launch leaves: the fp64 reference cast to fp32, untouched guards"""
    return _buffers(c, np.asarray(ref, dtype=np.float64).astype(np.float32), (c.ksplit if ksplit is None else ksplit) > 1)


def same_buffers(got, want):
    return (np.array_equal(got.out, want.out) and (got.ws_guard is None) == (want.ws_guard is None)
            and (got.ws_guard is None or np.array_equal(got.ws_guard, want.ws_guard)))


def emulate(c, x, w, off=None, in_max=None, ksplit=None, defect=None):
    """The launch in NumPy at fp32 (module docstring) -> Buffers.  x [B, cin, D, H, W], w [cout, cin, 3, 3, 3] (before the relu), off the
    offset or None, in_max (f16x2) the bound handed to the kernel (None: max x); ksplit: the K ranges of the launch (None: the case's;
    1: the same shape without a workspace); defect: one of DEFECTS."""
    n = c.ksplit if ksplit is None else ksplit
    assert defect is None or defect_applies(c, defect, n), (c, defect)
    f32 = np.float32
    B, cin, cout, D, H, W = c.batch, c.cin, c.cout, c.D, c.H, c.W
    dhw = D * H * W
    a = operand_of(x, off)
    wr = weights_of(c, np.ascontiguousarray(w, dtype=np.float32)).reshape(cout, cin, 27)
    A = a_bound(off, in_max_of(c, x, off) if in_max is None else in_max) if c.form == "x3f" else None
    pad = f32(0) - f32(off) if defect == "pad_minus_off" else f32(0)
    ap = np.full((B, cin, D + 3, H + 3, W + 3), pad, dtype=np.float32)        # one voxel in front, two behind (the tap_* defects)
    ap[:, :, 1:D + 1, 1:H + 1, 1:W + 1] = a
    pa, pw, (ia, iw) = cut(c, ap, wr, A)
    pw = [np.ascontiguousarray(p.reshape(cout, cin // 16, 16, 27).transpose(3, 1, 0, 2)) for p in pw]       # [tap][chunk][cout, 16]
    prods = [p for p in PRODUCTS[c.form] if defect != "drop_w%d_a%d" % p]
    ranges = k_ranges(c, n)
    nan = f32(np.nan)
    parts = []
    for k, (c0, c1) in enumerate(ranges):
        last_range = k == len(ranges) - 1
        part = np.full((B, cout, dhw), nan, dtype=np.float32)
        acc = np.zeros((B, cout, dhw), dtype=np.float32)
        start = c0 + 1 if (defect == "skip_first_chunk" and last_range) else c0
        for ch in range(start, c1):
            cs = slice(16 * ch, 16 * ch + 16)
            for rep in range(2 if (defect == "repeat_last_chunk" and k == 0 and ch == c1 - 1) else 1):
                for t in range(27):
                    dz, dy, dx = t // 9, (t // 3) % 3, t % 3
                    if t == 0 and ch == ranges[0][0]:
                        dz, dy, dx = dz + (defect == "tap_z"), dy + (defect == "tap_y"), dx + (defect == "tap_x")
                    tw = 4 if (defect == "stale_tap" and last_range and ch == c1 - 1 and t == 7) else t
                    shifted = {}                              # the tap's input planes [B, 16, voxels], one copy per piece
                    for qw, qa in prods:
                        if qa not in shifted:
                            shifted[qa] = pa[qa][:, cs, dz:dz + D, dy:dy + H, dx:dx + W].reshape(B, 16, dhw)
                        acc += np.matmul(pw[qw][tw, ch], shifted[qa])
            if (ch & 1) or ch + 1 == c1:
                av = (acc * f32(ia)) * f32(iw) if c.form == "x3f" else acc
                first = ch < c0 + 2 and defect != "first_flush_adds"
                part = av.copy() if first else part + av
                acc = np.zeros_like(acc)
        parts.append(part)
    if defect == "reduce_skips_last":
        parts = parts[:-1]
    out = parts[0]
    for p in parts[1:]:
        out = out + p
    out = out.reshape(B, cout, D, H, W)
    if defect == "colxy_swap":
        out = out.copy()
        for x0 in range(0, W - 7, TX):
            for y in range(H):
                if (y % TY) % 2 == 0:
                    lo, hi = out[:, :, :, y, x0:x0 + 4].copy(), out[:, :, :, y, x0 + 4:x0 + 8].copy()
                    out[:, :, :, y, x0:x0 + 4], out[:, :, :, y, x0 + 4:x0 + 8] = hi, lo
    bufs = _buffers(c, out, n > 1)
    if defect == "upper_block_past_cout":         # rows [max(cout, base + 32), base + 64) of the last item hold 0 (their packed weights are 0)
        base = cout // TM * TM
        r0, r1 = max(cout, base + 32) - cout, base + TM - cout
        (bufs.ws_guard if n > 1 else bufs.out[B * cout * dhw:])[r0 * dhw:r1 * dhw] = 0.0
    return bufs


# ------------------------------------------------------------------ operands
X3_THREE, X3_TWO, F16_TWO = LC.X3_THREE, LC.X3_TWO, LC.F16_TWO
POS = {"x3": (3, 8, 13), "x3f": (3, 13)}


def _seed(c, extra=0):
    return (c.batch * 7 + c.cin * 1009 + c.cout * 31 + c.D * 1013 + c.H * 101 + c.W * 11 + c.mode * 5 + FORMS.index(c.form) + 17 * extra) % (2 ** 31)


def probe_tap(co, ch, probe):
    """the tap of the weight probe: moves with the output channel, the chunk and the probe"""
    return (co + 7 * ch + 11 * probe) % 27


@functools.lru_cache(maxsize=None)
def integer_operands(c):
    """(x [B, cin, D, H, W], w [cout, cin, 3, 3, 3], off or None), fp32 and integer-valued (the module docstring); read-only, shared.
    Cases of one form and shape share them, with or without a workspace."""
    rng = np.random.RandomState(_seed(c))
    B, cin, cout, D, H, W = c.batch, c.cin, c.cout, c.D, c.H, c.W
    signed = c.mode == W_PLAIN
    chunks = chunks_of(c)
    vox = (B, chunks, D, H, W)
    a = rng.randint(-2 if signed else 0, 3, (B, cin, D, H, W)).astype(np.float32)
    w = rng.randint(-2, 3, (cout, cin, 27)).astype(np.float32)
    sign = lambda shape: (1 - 2 * rng.randint(0, 2, shape)).astype(np.float32) if signed else np.ones(shape, dtype=np.float32)
    av, wv = a.reshape(B, chunks, 16, D, H, W), w.reshape(cout, chunks, 16, 27)
    co, ch = np.meshgrid(np.arange(cout), np.arange(chunks), indexing="ij")

    def put(probe, pos, aval, wval):
        av[:, :, pos] = sign(vox) * aval
        wv[:, :, pos, :] = 0
        wv[co, ch, pos, probe_tap(co, ch, probe)] = sign((cout, chunks)) * wval

    if c.form == "x3":
        p3, p2, p1 = POS["x3"]
        put(0, p3, np.float32(X3_THREE), np.float32(1))
        put(1, p2, np.float32(X3_TWO), np.float32(X3_TWO))
        put(2, p1, np.float32(1), np.float32(X3_THREE))
    else:
        p2, p1 = POS["x3f"]
        put(0, p2, np.float32(F16_TWO) + rng.randint(1, 4, vox).astype(np.float32), rng.randint(1, 3, (cout, chunks)).astype(np.float32))
        put(1, p1, rng.randint(1, 3, vox).astype(np.float32), np.float32(F16_TWO) + rng.randint(1, 4, (cout, chunks)).astype(np.float32))
        av[0, 0, p2, 0, 0, 0] = F16_TWO + 3                    # max a = max w = 2^13 + 3 whatever the draw
        wv[0, 0, p1, probe_tap(0, 0, 1)] = F16_TWO + 3
    a[0, 0, 0, 0, 0] = 0.0 if not signed else a[0, 0, 0, 0, 0]             # the minimum of a is 0: off = min x
    a[-1, -1, -1, -1, -1], w[-1, -1, -1] = 2.0, 2.0                        # the corners carry data
    off = None if signed else INT_OFF
    x = a if signed else a + np.float32(INT_OFF)
    w = w.reshape(cout, cin, 3, 3, 3)
    for t in (x, w):
        t.setflags(write=False)
    return x, w, off


def in_max_of(c, x, off, loose=False):
    """the in_max handed to the f16x2 kernel: max x (W_PLAIN: max |x|), or the fp32 number that makes the bound 2^8 x larger"""
    if off is None:
        return float(np.float32(np.abs(x).max()) * np.float32(256.0 if loose else 1.0))
    span = float(np.float32(x.max()) - np.float32(off))
    return float(np.float32(np.float32(off) + np.float32(span * (256.0 if loose else 1.0))))


@functools.lru_cache(maxsize=None)
def random_operands(c):
    """(x, w, off or None), fp32 (the module docstring); read-only, shared"""
    rng = np.random.RandomState(_seed(c, 1))
    B, cin, cout, D, H, W = c.batch, c.cin, c.cout, c.D, c.H, c.W
    z, y, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    scale = (2.0 ** (-3.0 * ((z // 3 + y // 3 + xx // 3) % 8))).astype(np.float32)
    v = rng.standard_normal((B, cin, D, H, W)).astype(np.float32)
    w = (rng.standard_normal((cout, cin, 3, 3, 3)) * 0.2).astype(np.float32) * (2.0 ** rng.randint(-2, 3, (cout, 1, 1, 1, 1))).astype(np.float32)
    if c.mode == W_RELU:
        off = 0.0 if W % 2 else float(np.float32(0.37))
        x = np.float32(off) + np.maximum(v, np.float32(0)) * scale
        x[..., :min(4, W // 2)] = np.float32(off)
        w[cout // 2] = -np.abs(w[cout // 2])
    else:
        off = None
        x = v * scale
        w[cout // 2] = 0
    x = np.ascontiguousarray(x, dtype=np.float32)
    for t in (x, w):
        t.setflags(write=False)
    return x, w, off


# ------------------------------------------------------------------ reference and bound
def _tensors(c, x, w, off):
    """(a, W or relu(W)) as fp32 tensors (copies: the shared operands are read-only)"""
    return torch.from_numpy(np.array(operand_of(x, off), dtype=np.float32)), torch.from_numpy(np.array(weights_of(c, np.asarray(w)), dtype=np.float32))


def reference(c, x, w, off):
    """(y, S) fp64 tensors: the conv of a = fl32(x - off) with W or relu(W), and the conv of their absolute values"""
    a, wr = _tensors(c, x, w, off)
    return DC.conv64(a, wr, 3), DC.conv64(a.abs(), wr.abs(), 3)


@functools.lru_cache(maxsize=None)
def integer_reference(c):
    """(y, S) of the integer operands, computed once and shared"""
    return reference(c, *integer_operands(c))


def n_roundings(c, ksplit=None):
    """n of the bf16x3 bound (the module docstring)"""
    return 324 * chunks_of(c) + pairs_of(c) + (c.ksplit if ksplit is None else ksplit) - 1


def bound(c, x, w, off, in_max=None, ksplit=None):
    """(y, E, S): the fp64 reference, the per-element error bound and S = sum |a| |w|, fp64 tensors"""
    y, S = reference(c, x, w, off)
    if c.form == "x3":
        n = n_roundings(c, ksplit)
        g = n * 2.0 ** -24 / (1 - n * 2.0 ** -24)
        return y, (1 + 2.0 ** -6) * g * S + (2.0 ** -20 + 2.0 ** -28) * S + 2.0 ** -24 * y.abs(), S
    a, wr = _tensors(c, x, w, off)
    A = a_bound(off, in_max_of(c, x, off) if in_max is None else in_max)
    C, Sa, Sb, n = F16C.terms(F16C.conv3d_op, a, wr)
    return y, F16C.bound("x3f", c.cin, C, Sa, Sb, n, A, w_bound(wr.numpy()), y), S
