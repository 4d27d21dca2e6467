"""The case table of the fp32 RoIAlign3D forward (csrc/roi_align3d.hip: roi_align3d_fwd_v3_kernel, roi_align3d_fwd_sep_kernel,
roi_align3d_kernel<false>, roi_untabled_range<false>, roi_class_kernel, roi_tap_table_kernel), its fp64 reference, its error bound and a
host restatement of the routing.  No tests live here: tests/test_roi_align_forward_cases_host.py checks the reference against the C
oracle, proves from route() that the table reaches every code path under every hand-over kind, and shows which wrong forwards the bound
rejects that the suite's older criterion (1e-5 * max |f|) accepted; tests/test_gpu_roi_align_forward.py runs the kernels.  The sample
arithmetic (axis_table, roi_geometry, _matrices) is the backward module's, tests/roi_align_backward_cases.py, with z_limit = -1.0.

The operation (roi_align_kernel_3d.cu:16-151 as this library implements it).  A RoI row is (batch, x1, y1, z1, x2, y2, z2) in image
voxels.  Per axis, in fp32 and in exactly this order (see the backward module's docstring; make_sample of csrc/roi_align3d_geom.h):
    start = r1 * scale, end = r2 * scale, roi = fmaxf(end - start, 1), bin = roi / A, grid = ratio > 0 ? ratio : (int)ceilf(roi / A)
    c = start + p * bin;  c = c + (i + .5f) * bin / grid;   valid = !((double)c < -1.0 || c > dim)        on ALL THREE axes
    if (c <= 0) c = 0;  lo = (int)c;  if (lo >= dim - 1) { hi = lo = dim - 1; c = lo; } else hi = lo + 1;  l = c - lo,  h = (float)(1. - l)
and with count = grid_z * grid_y * grid_x (ALL samples, valid or not) the output element o = (r, c, ph, pw, ps) is
    out[r, c, ph, pw, ps] = 1 / count * sum over the samples (iz, iy, ix) of bin (ps, ph, pw) whose three axes are valid of
                            sum over the 8 corners of  wz * wy * wx * f[batch, c, z, y, x]          (w = h on voxel lo, l on voxel hi)
written at flat index (ph * AW + pw) * AS + ps of the [R, C, AS, AH, AW] tensor: the memory order is (ph, pw, ps), NOT the tensor's.
Everything here is shaped [R, C, AH, AW, AS] for that reason.  Validity and weights are separable per axis, so the reference is three
matrices [A, dim] per RoI (M[p, d] = sum over the valid sub-samples of bin p of the weight on voxel d, from the fp32 table values h
and l) and one contraction in fp64.  It returns per element
    ref_o   the fp64 value,
    A_o     sum of |w f| / count over the valid samples' corners (weights are >= 0, so every fp32 form below shares this A_o),
    n_o     8 * the number of valid samples of the bin.

Error bound, per output element (derived, not fitted), u = 2^-24:
    |got_o - ref_o| <= (n_o + K) * u * A_o,   K = 4 on every path,          and got_o == 0.0 exactly where A_o == 0.
To first order the error of any of the forms is at most (the largest number of roundings on the way of one term w f into the result)
* u * A_o: all weights are >= 0, so every partial sum of every pass is bounded by the partial sum of the |terms|.  The table values
lo, hi, l, h, valid are the same fp32 numbers in every kernel and here; in particular h = fl(1 - l) IS the operation's weight (the
rounding of 1 - l is inside the table, on both sides, and costs nothing).  Let vz, vy, vx be the valid sub-samples of the bin per axis:
n_o = 8 vz vy vx, and A_o > 0 needs n_o >= 8.  Longest chain per path:
  exact (roi_exact_forward_range, roi_untabled_range<false>, roi_align3d_kernel<false>, the oracle):  w = fl(fl(wz wy) wx) 2, the
        product with f 1, the left-to-right sum of the sample's 8 corners <= 7, `acc += val` <= n_o / 8 - 1 (an invalid sample adds an
        exact 0, the first valid one is added to 0), the divide 1:  n_o / 8 + 10  <=  n_o + 3  at n_o >= 8.                     needs K >= 3
  sep, table-driven passes (generic staged and the whole-workgroup cooperative tier):  per pass the product 1, h f_lo + l f_hi 1, the
        accumulation over the axis' valid sub-samples <= v - 1; then fl(1 / count) 1 and the multiply 1:
        vx + vy + vz + 5  <=  8 vx vy vz = n_o.                                                                                  needs K >= 0
  sep, register taps (staged and global-x):  per pass the product 1 and two levels of adds 2; on z the weight is fl(h * fl(1 / count)),
        2 more:  3 * 3 + 2 = 11  <=  n_o + 3.                                                                                    needs K >= 3
  v3 (all four forms):  the fold adds up to four weights onto one voxel, <= 3 roundings per axis, and only on an axis with two valid
        sub-samples (one valid sample puts h and l on two voxels, or, clamped at dim - 1, adds l = 0); its 0.125 is a power of two,
        exact; per pass the product 1 and two levels of adds 2:  9 + 3 * (axes with v = 2) against n_o = 8 * 2^(those axes):
        9, 12, 15, 18 against 8, 16, 32, 64.                                                                                     needs K >= 1
No path needs a constant of its own: K = 3 + 1, the 1 for the second-order terms (chain^2 u: 0.03 roundings for the longest chain of the
table, 739 at grid 9) and the reference's own fp64 roundings.  No product leaves the normal range: a weight is zero or >= 2^-23 or so and
the quietest channel's values are around 1e-7 of the loudest, far above 1e-38 * 2^24 even cubed and divided by 729.
A_o == 0 means every term has a zero factor (an invalid sample is skipped or carries weight 0; features are finite), and a sum of fp32
zeros is zero.  Non-finite features are outside the contract (v3 multiplies neighbouring voxels by weight 0).
The matrix-core form (m3d_roi_align3d_forward_ws2 / _ws3 with feat_absmax) is NOT covered here: tests/f16x2_contract.py, row roi_gemm.

Largest |got - ref| / bound per case on the MI355X: recorded in DESIGN.md (RoIAlign3D); tests/test_gpu_roi_align_forward.py prints them
(pytest -s).
"""
import collections
import functools

import numpy as np

import roi_align_backward_cases as T

F32 = np.float32
U = T.U
K_BOUND = 4
K_MAX_TABLE = T.K_MAX_TABLE
K_SEP_LDS_FLOATS = 8192       # csrc/roi_align3d.hip kSepLdsFloats
K_SEP_STAGE_MAX = 1536        # kSepStageMax
K_SLICE = K_SEP_LDS_FLOATS // 4
M3D_EINVAL, M3D_EUNSUPPORTED = -1, -4
# the class markers roi_class_kernel writes at element 0 of every 8th channel of a RoI's output (quiet NaNs with a payload)
MARKERS = {"declined": 0x7FC0DEAD, "small": 0x7FC05A11, "medium": 0x7FC03ED0, "gemm4": 0x7FC06E34, "gemm8": 0x7FC06E38}

Case = T.Case                 # id shape bins ratio R scale
BIG = (16, 16, 40)            # (S, H, W) of the maps that hold every tier of sub-volume

CASES = (
    Case("marks_c64", (2, 64) + BIG, (7, 7, 7), 2, 48, 0.125),            # C % 32 == 0, ccpb = 8: hand-over through the markers
    Case("pred_c40", (2, 40) + BIG, (7, 7, 7), 2, 24, 0.125),             # v3 chunks 32 + 8 (dual loop ends evenly), sep chunks of 5
    Case("pred_c37", (2, 37) + BIG, (7, 7, 7), 2, 32, 0.125),             # v3 chunks 32 + 5 (waves with 2, 1, 1, 1 channels), sep chunks 5 .. 2; 10 % zeros
    Case("pred_c8", (1, 8) + BIG, (7, 7, 7), 2, 12, 0.125),               # one chunk of 8 everywhere
    Case("bins3", (2, 9, 6, 9, 11), (3, 3, 3), 2, 20, 0.125),             # table-driven staged passes
    Case("noncubic", (2, 9, 6, 9, 11), (2, 3, 4), 3, 20, 0.125),          # the output's (ph, pw, ps) order shows
    Case("adaptive_tabled", (1, 6) + BIG, (7, 7, 7), 0, 14, 0.125),       # grids 1..9, different per axis; cooperative and exact tiers
    Case("adaptive_222", (2, 37) + BIG, (7, 7, 7), 0, 16, 0.125),         # ratio 0 and every grid (2, 2, 2): the register-tap tiers
    Case("adaptive_untabled", (1, 3, 12, 14, 16), (7, 7, 7), 0, 4, 0.125),  # grid 12: roi_untabled_range<false> next to tabled RoIs
    Case("avg_wrapper", (1, 8, 5, 7, 9), (8, 8, 8), 2, 10, 0.125),        # the A + 1 geometry of RoIAlignAvg_3d / RoIAlignMax_3d
    # v3 chunks 32 + 11: waves with 3, 3, 3, 2 channels - a partial iteration of the two-channel loop AFTER a full one, which needs a
    # last chunk of 9 .. 12 channels under the predicate hand-over and which none of 64, 40, 37, 8 gives (last of the table: seeds)
    Case("pred_c43", (2, 43) + BIG, (7, 7, 7), 2, 16, 0.125),
)
BY_ID = {c.id: c for c in CASES}
V3_CASES = tuple(c for c in CASES if c.ratio == 2 and c.bins == (7, 7, 7))
SHIPPED = "pred_c8"           # the shipped geometry at the smallest size: the wrappers' case


# every (label, hand-over kind) the code has; tests/test_roi_align_forward_cases_host.py proves the table reaches each
V3_LABELS = ("v3.w4.dual", "v3.w4.single", "v3.w2", "v3.w1")
SEP_COMPLEMENT_LABELS = ("sep.zero", "sep.reg_staged", "sep.reg_globalx", "sep.coop", "sep.exact")
REQUIRED = frozenset([(lb, h) for lb in V3_LABELS + SEP_COMPLEMENT_LABELS for h in ("marks", "predicate")] +
                     [(lb, "none") for lb in SEP_COMPLEMENT_LABELS + ("sep.untabled", "sep.generic_staged")])


def case_id(c):
    return c.id


def _box(b, z, y, x):
    """a RoI row whose 7 x 2 samples per axis reach exactly the voxels [v0, v0 + e) for each (v0, e) = z, y, x: the first sample at
    v0 + 0.3, the last at v0 + e - 1.4 (its high corner is v0 + e - 1), in image voxels at scale 0.125"""
    row = [b]
    ends = []
    for v0, e in (x, y, z):
        bin_ = (e - 1.7) / 6.5
        start = v0 + 0.3 - 0.25 * bin_
        row.append(start * 8)
        ends.append((start + 7 * bin_) * 8)
    return row + ends


def engineered(b=0):
    """one RoI per tier of the shipped geometry on a BIG map, in the order of ENGINEERED"""
    return [
        _box(b, (2, 4), (3, 4), (5, 4)),          # 4^3: per_ch 583, two channels at a time
        _box(b, (1, 8), (2, 8), (3, 8)),          # 8^3: 1563, one channel, 4 waves
        _box(b, (2, 12), (2, 12), (20, 12)),      # 12^3: 3535, 2 waves
        _box(b, (0, 16), (0, 16), (10, 16)),      # 16^3: 6883, 1 wave
        _box(b, (5, 3), (6, 4), (2, 36)),         # 3 x 4 x 36: bins 5.3 voxels wide in x, declined; staged
        _box(b, (4, 6), (3, 7), (0, 40)),         # 6 x 7 x 40: sub 1680 > 1536; global-x
        _box(b, (2, 12), (1, 14), (3, 36)),       # 12 x 14 x 36: n1 + n2 = 1764, per_ch 7812; cooperative
        _box(b, (0, 16), (0, 16), (4, 32)),       # 16 x 16 x 32: per_ch > 8192; exact order inside the sep kernel
    ]


ENGINEERED = ("v3.w4.dual", "v3.w4.single", "v3.w2", "v3.w1", "sep.reg_staged", "sep.reg_globalx", "sep.coop", "sep.exact")


@functools.lru_cache(maxsize=None)
def rois(c):
    rs = np.random.RandomState(5000 + CASES.index(c))
    B = c.shape[0]
    k = [r for b in range(B) for r in T._classes(c, b)]
    if c.id == "marks_c64":
        rows = engineered(0) + [engineered(1)[0], engineered(1)[6]] + k
        rows += [[1, 10, 14, 6, 52, 40, 37]] * 2                                         # the same RoI twice
    elif c.id == "pred_c40":
        rows = engineered(0) + k[:14]
    elif c.id == "pred_c37":
        rows = engineered(1) + k[14:]
    elif c.id == "pred_c43":
        rows = engineered(0) + [engineered(1)[0], engineered(1)[1], k[0], k[8], k[14 + 12], k[14 + 11]]
    elif c.id == "pred_c8":
        rows = engineered(0) + [k[8], k[12], k[11], k[7]]                                # fully outside, z band, whole map, malformed
    elif c.id in ("bins3", "noncubic"):
        rows = [k[i] for i in (12, 26, 13, 7, 8, 9, 10, 11, 25)]
    elif c.id == "adaptive_tabled":
        rows = [list(r) for r in T.rois(T.BY_ID["adaptive_tabled"])[:8]]                 # grids 1..9, z band, sub-voxel, malformed, outside
        rows += [[0, 0, 0, 0, 320, 128, 128],                                            # the whole map: grids (3, 3, 6), 10240 voxels
                 [0, 40, 16, 24, 280, 112, 104]]                                         # 10 x 12 x 30 voxels: grids (2, 2, 5)
        rows += T._random(c, rs, c.R - len(rows), 30.0, 480.0)
    elif c.id == "adaptive_222":
        # every size in (7, 14] feature voxels = (56, 112] image voxels: grid = ceil(size / 7) = 2 on every axis
        rows = [[0, 8, 8, 8, 68, 68, 68],                                                # 9^3 voxels
                [0, -40, -40, -40, 24, 24, 24],                                          # cut by three low faces: a small sub-volume
                [1, 8, 8, 100, 120, 120, 212],                                           # 15^3
                [0, 16, 16, 16, 108, 108, 108],
                [1, 200, 20, 10, 288, 90, 80],
                [0, -20, 30, -6, 60, 100, 70],                                           # z samples in the band [-1, -0.1): kept
                [1, 260, 70, 70, 360, 170, 170],                                         # cut by three high faces
                [0, 30, 30, 30, 90, 130, 140]]
        rows += T._random(c, rs, c.R - len(rows), 57.0, 111.0)
    elif c.id == "adaptive_untabled":
        rows = [list(r) for r in T.rois(T.BY_ID["adaptive_untabled"])]
    elif c.id == "avg_wrapper":
        rows = [k[i] for i in (12, 0, 0, 7, 8, 9)]
    rows += T._random(c, rs, c.R - len(rows))
    out = np.array(rows, np.float64).astype(F32)
    assert out.shape == (c.R, 7), (c.id, out.shape)
    out.setflags(write=False)
    return out


QUIET = (1e-6, 3e-7)          # the last two channels' scales relative to the loudest channel's


@functools.lru_cache(maxsize=None)
def features(c):
    """seeded randn with a per-channel scale exp(randn); the last two channels are QUIET (an error there is invisible under a tolerance
    relative to the tensor's largest value); `pred_c37`: about 10 % exact zeros"""
    rs = np.random.RandomState(6000 + CASES.index(c))
    C = c.shape[1]
    scale = np.exp(rs.randn(C))
    scale[C - 2:] = scale.max() * np.array(QUIET)
    f = rs.randn(*c.shape) * scale[None, :, None, None, None]
    if c.id == "pred_c37":
        f[rs.uniform(0, 1, f.shape) < 0.1] = 0.0
    f = f.astype(F32)
    f.setflags(write=False)
    return f


# ---------------------------------------------------------------------------------------------- the fp64 reference
Result = collections.namedtuple("Result", "ref A n geoms")       # arrays [R, C, AH, AW, AS]: the output's memory order


def _drop_fourth(M, t):
    """the v3 fold without its fourth tap: per bin, the weight on voxel base + 3 (base = the lowest voxel of the bin's valid samples)"""
    for p in range(M.shape[0]):
        if t.valid[p].any():
            d = int(t.lo[p][t.valid[p]].min()) + 3
            if d < M.shape[1]:
                M[p, d] = 0.0


def reference(feat, rois_, shape, bins, scale, ratio, z_limit=-1.0, count_plus=0, ignore_batch=False, hi_is_lo=False,
              drop_fourth_tap=False):
    """fp64 forward with A_o, n_o (module docstring) and the per-RoI tables.  The keyword arguments after `ratio` are wrong forwards of
    the sensitivity test: the backward's z limit, count off by one, every RoI on batch item 0, both corners of an axis on the low voxel,
    the fold's fourth tap dropped."""
    B, C, S, H, W = shape
    AS, AH, AW = bins
    rois_ = np.asarray(rois_, F32)
    R = rois_.shape[0]
    assert feat.shape == tuple(shape) and rois_.shape == (R, 7)
    f = np.asarray(feat, np.float64)
    fa = np.abs(f)
    ref, A, n = np.zeros((R, C, AH, AW, AS)), np.zeros((R, C, AH, AW, AS)), np.zeros((R, 1, AH, AW, AS))
    geoms = []
    for r in range(R):
        g = T.roi_geometry(rois_[r], scale, bins, ratio, (S, H, W), z_limit, hi_is_lo)
        geoms.append(g)
        Ms = [T._matrices(t, a, d)[0] for t, a, d in zip(g.axes, bins, (S, H, W))]
        if drop_fourth_tap:
            for M, t in zip(Ms, g.axes):
                _drop_fourth(M, t)
        Mz, My, Mx = Ms
        b = 0 if ignore_batch else g.batch
        assert 0 <= b < B
        for src, dst in ((f, ref), (fa, A)):
            a = src[b] @ Mx.T                                               # [C, S, H, AW]
            a = np.einsum("czyk,jy->czjk", a, My)                           # [C, S, AH, AW]
            dst[r] = np.einsum("czjk,iz->cjki", a, Mz) / float(g.count + count_plus)
        vz, vy, vx = (t.valid.sum(1) for t in g.axes)
        n[r, 0] = 8.0 * vy[:, None, None] * vx[None, :, None] * vz[None, None, :]
    return Result(ref, A, np.broadcast_to(n, ref.shape), geoms)


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """the reference of a case of the table: computed once, shared, read-only"""
    res = reference(features(c), rois(c), c.shape, c.bins, c.scale, c.ratio)
    for a in (res.ref, res.A):
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def oracle_of(c):
    """the C oracle (fp32, the reference's operation order) on a case of the table: computed once, shared, read-only"""
    import oracle as O
    out = O.roi_align_3d_forward(features(c), rois(c), *c.bins, c.scale, c.ratio)
    out.setflags(write=False)
    return out


def bound(res):
    return (res.n + K_BOUND) * U * res.A


Verdict = collections.namedtuple("Verdict", "outside nonzero worst where")


def compare(got, res):
    """got (R * C * bins values in the output's memory order, any shape) against a Result: the number of elements outside the bound (a NaN
    is outside), the number that are not 0.0 where A_o == 0, the largest |got - ref| / bound over the elements with A_o > 0 and its index
    (r, c, ph, pw, ps)"""
    got = np.asarray(got, np.float64)
    assert got.size == res.ref.size, (got.shape, res.ref.shape)
    got = got.reshape(res.ref.shape)
    bd = bound(res)
    err = np.abs(got - res.ref)
    live = res.A > 0
    ratio = np.zeros_like(err)
    ratio[live] = err[live] / bd[live]
    ratio[np.isnan(ratio)] = np.inf
    where = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return Verdict(int((~(err <= bd)).sum()), int((got[~live] != 0.0).sum()), float(ratio[where]), tuple(int(i) for i in where))


def describe(v):
    return "%d elements outside the bound, %d not 0.0 where no sample is valid; largest err / bound %.4f at (r, c, ph, pw, ps) = %s" % (
        v.outside, v.nonzero, v.worst, v.where)


def old_criterion(got, res, feat):
    """what tests/test_gpu_ops.py asks of the fast forms: max |got - ref| <= 1e-5 * max |f| over the whole tensor"""
    return bool(np.abs(np.asarray(got, np.float64).reshape(res.ref.shape) - res.ref).max() <= 1e-5 * np.abs(feat).max())


# ---------------------------------------------------------------------------------------------- what launch() does with a RoI
Route = collections.namedtuple("Route", "label handover nw dual chunks wave_channels ragged even lone grid sub")


def _range(t):
    return (int(t.lo[t.valid].min()), int(t.hi[t.valid].max())) if t.valid.any() else None


def _fold_ok(t):
    """fold_bin's ok-rule for the 7 bins of an axis at grid 2: every tap of the bin's valid samples within base .. base + 3"""
    for p in range(7):
        v = t.valid[p]
        if v.any() and int(t.hi[p][v].max()) - int(t.lo[p][v].min()) > 3:
            return False
    return True


def _chunks(C, per):
    return [(c0, min(C, c0 + per)) for c0 in range(0, C, per)]


def _wave_channels(chunks, nw):
    """channels each working wave takes in each chunk (`for c = c0 + wave; c < c1; c += nw`)"""
    return [max(0, -(-(c1 - c0 - w) // nw)) for c0, c1 in chunks for w in range(nw)]


def route(roi_row, C, R, shape, bins, ratio, scale):
    """Which code path of m3d_roi_align3d_forward / _forward_ws (no feat_absmax) computes this RoI: launch() and the kernels restated in
    integers and fp32 NumPy.  label: v3.w4.dual / v3.w4.single / v3.w2 / v3.w1 (roi_align3d_fwd_v3_kernel) or sep.zero / sep.untabled /
    sep.generic_staged / sep.reg_staged / sep.reg_globalx / sep.coop / sep.exact (roi_align3d_fwd_sep_kernel); handover: how the two
    launches of the shipped geometry agree on the RoI, `marks` (roi_class_kernel's markers in the output) or `predicate` (both repeat the
    test), `none` for every other geometry (one launch); nw, dual: working waves and v3_run<true>; chunks: the channel ranges of the
    workgroups that compute it; wave_channels: the channels a wave takes of a chunk, all values that occur; ragged / even / lone, of
    v3_run<true>'s two-channel loop: some wave has an odd number >= 3 of channels, so a PARTIAL iteration follows a full one - the full one
    ends with `if (!more) first = true`, the partial one waits for everything, fetches one sub-volume and runs its second channel's passes
    on the buffer the pair before left, stores masked / some wave's loop ends on a full pair / some wave has ONE channel: its only iteration
    is partial but also the first, with the ordinary first wait."""
    B, _, S, H, W = shape
    AS, AH, AW = bins
    g = T.roi_geometry(np.asarray(roi_row, F32), scale, bins, ratio, (S, H, W), -1.0)
    v3 = ratio == 2 and bins == (7, 7, 7)
    cchunks = 1
    while R * cchunks < 4096 and cchunks * 8 < C:
        cchunks *= 2
    ccpb = -(-C // cchunks)
    marks = C % 32 == 0 and ccpb % 8 == 0
    handover = ("marks" if marks else "predicate") if v3 else "none"
    sep_chunks = _chunks(C, ccpb) if v3 else _chunks(C, max(T.chunk_sizes(R, C)))

    def sep(label, sub=0):
        return Route(label, handover, 4, False, sep_chunks, sorted(set(_wave_channels(sep_chunks, 4))), False, False, False, g.grid, sub)

    if any(a * k > K_MAX_TABLE for a, k in zip(bins, g.grid)):
        assert not v3
        return sep("sep.untabled")
    rng = [_range(t) for t in g.axes]
    if any(r is None for r in rng):
        return sep("sep.zero")
    ez, ey, ex = (r[1] - r[0] + 1 for r in rng)
    sub = ez * ey * ex
    if v3:
        subp = (sub + 3 + 63) // 64 * 64
        per_ch = subp + ez * ey * 7 + (ey + 3) * 49
        if per_ch <= K_SEP_LDS_FLOATS and all(_fold_ok(t) for t in g.axes):
            nw = 4
            while nw > 1 and per_ch > K_SEP_LDS_FLOATS // nw:
                nw >>= 1
            dual = 2 * per_ch <= K_SEP_LDS_FLOATS // nw
            chunks = ([(0, C)] if nw == 4 else _chunks(C, 8)) if marks else _chunks(C, 32)
            wc = _wave_channels(chunks, nw)
            label = "v3.w4.dual" if dual else ("v3.w4.single" if nw == 4 else "v3.w%d" % nw)
            assert not dual or nw == 4
            return Route(label, handover, nw, dual, chunks, sorted(set(wc)), dual and any(m >= 3 and m % 2 == 1 for m in wc),
                         dual and any(m > 0 and m % 2 == 0 for m in wc), dual and 1 in wc, g.grid, sub)
    n1, n2 = ez * ey * AW, ez * AH * AW
    per_ch = sub + n1 + n2
    reg_taps = g.grid == (2, 2, 2) and bins == (7, 7, 7)
    staged = sub <= K_SEP_STAGE_MAX and per_ch + 343 <= K_SLICE
    globalx = not staged and reg_taps and n1 + n2 + 343 <= K_SLICE
    if staged:
        return sep("sep.reg_staged" if reg_taps else "sep.generic_staged", sub)
    if globalx:
        return sep("sep.reg_globalx", sub)
    return sep("sep.exact" if per_ch > K_SEP_LDS_FLOATS else "sep.coop", sub)


@functools.lru_cache(maxsize=None)
def routes_of(c):
    return tuple(route(r, c.shape[1], c.R, c.shape, c.bins, c.ratio, c.scale) for r in rois(c))


def tap_table(r, scale, dims, B):
    """roi_tap_table_kernel's record of one RoI row: int32 [3, 14, 4] = (lo, hi, bits(h * valid), bits(l * valid)) per axis (z, y, x) and
    sample 2 p + i, and the clamped batch index"""
    g = T.roi_geometry(np.asarray(r, F32), scale, (7, 7, 7), 2, dims, -1.0)
    tab = np.zeros((3, 14, 4), np.int32)
    for a, t in enumerate(g.axes):
        tab[a, :, 0] = t.lo.ravel()
        tab[a, :, 1] = t.hi.ravel()
        tab[a, :, 2] = np.where(t.valid, t.h, F32(0)).astype(F32).ravel().view(np.int32)
        tab[a, :, 3] = np.where(t.valid, t.l, F32(0)).astype(F32).ravel().view(np.int32)
    return tab, min(max(g.batch, 0), B - 1)
