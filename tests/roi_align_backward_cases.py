"""The case table of the RoIAlign3D backward (csrc/roi_align3d.hip: roi_align3d_kernel<true>, roi_untabled_range<true>), its fp64 reference
and its error bound.  No tests live here: tests/test_roi_align_backward_cases_host.py checks the reference against the C oracle, proves
from the reference's own sample tables that the table reaches what it is for, and shows that the bound separates five wrong backwards
from the right one; tests/test_gpu_roi_align_backward.py runs the kernel and the autograd wrappers of m3d.compat over it.

The operation (roi_align_kernel_3d.cu:180-338 as this library implements it).  A RoI row is (batch, x1, y1, z1, x2, y2, z2) in image
voxels.  Per axis, in fp32 and in exactly this order (the file is built with -ffp-contract=off, the order is the contract with
oracle/m3d_oracle.c):
    start = r1 * scale, end = r2 * scale, roi = fmaxf(end - start, 1), bin = roi / A, grid = ratio > 0 ? ratio : (int)ceilf(roi / A)
    c = start + p * bin;  c = c + (i + .5f) * bin / grid                                 bin p < A, sub-sample i < grid
    valid = !((double)c < limit || c > dim)             limit = -0.1 on z and -1.0 on y and x (the forward has -1.0 on all three)
    if (c <= 0) c = 0;  lo = (int)c;  if (lo >= dim - 1) { hi = lo = dim - 1; c = lo; } else hi = lo + 1
    l = c - lo,  h = (float)(1. - l)                    weight h goes to voxel lo, weight l to voxel hi
and with count = grid_z * grid_y * grid_x every sample whose three axes are valid adds, for each of its 8 corners,
    grad[batch, ch, z, y, x] += top[r, ch, ps, ph, pw] * wz * wy * wx / count
`top` is read at ps * AH * AW + ph * AW + pw - the natural order of a [R, C, AS, AH, AW] tensor, NOT the (ph, pw, ps) order the forward
writes.  Validity and weights are separable per axis, so the reference below is three matrices [A, dim] per RoI
(M[p, d] = sum over the valid sub-samples of bin p of the weight that lands on voxel d) and one contraction in fp64.

Error bound, per element e of the gradient (derived, not fitted):
    |got_e - ref_e| <= (n_e + 8) * 2^-24 * A_e,            and got_e == 0.0 exactly where A_e == 0
    A_e = sum of |contribution| over the adds that land on e (fp64)
    n_e = the number of atomic adds that land on e (the two corners of an axis clamped at dim - 1 are two adds to one address)
Derivation, with u = 2^-24.  The kernel adds a = fl(fl(t * w) / count) with w = fl(fl(wz * wy) * wx): four roundings, so
|a - t wz wy wx / count| <= 4u |t wz wy wx / count| to first order (the table values wz, wy, wx are the same fp32 numbers in the kernel
and here; count is a small integer, exact in both).  The n_e values then meet in fp32 atomic adds in an order nobody chooses; recursive
summation in ANY order is off by at most (n_e - 1) u sum |a| to first order.  Together (n_e + 3) u A_e; the constant 8 leaves room
for the second-order terms and for the reference's own fp64 roundings.  The second-order term of the summation is n_e u relative to the
first (0.6 % at n_e = 10^5, the densest element of `table_edge`): a worst-case analysis would add it, a measured error grows like
sqrt(n_e) u and stays far inside.  No product underflows: in this table a weight is zero or >= 2^-21 and |top| is zero or
>= 4e-7, so the smallest non-zero add is above 1e-29.
A_e == 0 means every add to e has a zero factor, and a sum of fp32 zeros is zero.

Largest |got - ref| / bound per case on the MI355X: recorded in DESIGN.md (RoIAlign3D); tests/test_gpu_roi_align_backward.py prints them
(pytest -s).
"""
import collections
import functools

import numpy as np

F32 = np.float32
U = 2.0 ** -24
K_BOUND = 8
K_MAX_TABLE = 64              # csrc/roi_align3d.hip kMaxTable: A * grid per axis the LDS tables take
M3D_EUNSUPPORTED = -4

Case = collections.namedtuple("Case", "id shape bins ratio R scale")

CASES = (
    Case("shipped", (2, 37, 6, 9, 11), (7, 7, 7), 2, 48, 0.125),          # 4 chunks (10, 10, 10, 7), 14 loop trips, both batch items
    Case("wide_c", (1, 256, 4, 5, 6), (7, 7, 7), 2, 9, 0.125),            # 16 chunks of 16 channels
    Case("narrow_c", (1, 5, 5, 6, 7), (3, 3, 3), 2, 1, 0.125),            # one chunk, C < 16, one RoI
    Case("many_rois", (1, 24, 3, 4, 5), (2, 2, 2), 2, 2100, 0.125),       # R >= 2048: one chunk although C > 16
    Case("noncubic_a", (2, 9, 6, 9, 11), (2, 3, 4), 3, 20, 0.125),        # top strides
    Case("noncubic_b", (2, 9, 6, 9, 11), (4, 2, 3), 2, 20, 0.125),        # top strides, the other order
    Case("table_edge", (1, 4, 6, 7, 8), (7, 7, 7), 9, 4, 0.125),          # A * ratio = 63: the last size the tables take
    Case("adaptive_tabled", (1, 6, 8, 10, 12), (7, 7, 7), 0, 12, 0.125),  # grids 1..9, different per axis
    Case("adaptive_untabled", (1, 3, 12, 14, 16), (7, 7, 7), 0, 4, 0.125),  # grid 12: roi_untabled_range<true>, next to tabled RoIs
    Case("avg_wrapper", (1, 8, 5, 7, 9), (8, 8, 8), 2, 10, 0.125),        # the A + 1 geometry of RoIAlignAvg_3d / RoIAlignMax_3d
)
BY_ID = {c.id: c for c in CASES}

# the one call of the table that must be refused: 7 * 10 = 70 table entries per axis at a FIXED ratio (an adaptive grid of that size takes
# the untabled path; a fixed one is an unsupported configuration) -> M3D_EUNSUPPORTED, nothing launched
REFUSED = dict(shape=(1, 4, 6, 7, 8), bins=(7, 7, 7), ratio=10, scale=0.125,
               rois=np.array([[0, 8, 8, 8, 40, 40, 30]], F32))


def case_id(c):
    return c.id


def _extent(c):
    """(x, y, z) size of the map in image voxels"""
    _, _, S, H, W = c.shape
    return np.array([W, H, S]) / c.scale


def _classes(c, b):
    """one RoI of every class on batch item b, placed relative to the map: inside, straddling each of the six faces, malformed, fully
    outside, mostly outside, sub-voxel, the whole map and more, and the two z-band RoIs (z samples in [-1, -0.1): the forward's rule
    keeps them, the backward's drops them; their x and y samples in the same band stay valid)"""
    ex, ey, ez = _extent(c)
    return [
        [b, 0.2 * ex, 0.2 * ey, 0.2 * ez, 0.7 * ex, 0.7 * ey, 0.7 * ez],                 # inside
        [b, -12, 0.25 * ey, 0.2 * ez, 20, 0.7 * ey, 0.6 * ez],                           # x low face
        [b, ex - 18, 0.25 * ey, 0.2 * ez, ex + 12, 0.7 * ey, 0.6 * ez],                  # x high face
        [b, 0.2 * ex, -12, 0.2 * ez, 0.6 * ex, 20, 0.6 * ez],                            # y low
        [b, 0.2 * ex, ey - 12, 0.2 * ez, 0.6 * ex, ey + 12, 0.6 * ez],                   # y high
        [b, 0.2 * ex, 0.25 * ey, -12, 0.6 * ex, 0.7 * ey, 20],                           # z low
        [b, 0.2 * ex, 0.25 * ey, ez - 12, 0.6 * ex, 0.7 * ey, ez + 12],                  # z high
        [b, 40, 30, 20, 30, 50, 40],                                                     # malformed: x2 < x1
        [b, 4000, 4000, 4000, 4000, 4000, 4000],                                         # fully outside
        [b, -30, -30, -30, 6, 6, 6],                                                     # mostly outside
        [b, 33, 34, 21, 35, 36, 23],                                                     # sub-voxel: the size clamps to 1
        [b, -10, -10, -10, ex + 12, ey + 13, ez + 12],                                   # the whole map and more
        [b, 20, 30, -6, 60, 70, 10],                                                     # z band
        [b, -6, -6, -6, 10, 10, 10],                                                     # z band, x and y in the band too
    ]


def _random(c, rs, n, smin=1.0, smax=60.0):
    """n seeded RoIs: centres up to 8 voxels outside the map on every side (they straddle faces), sizes smin..smax image voxels"""
    B = c.shape[0]
    ctr = rs.uniform(-8, 1, (n, 3)) + rs.uniform(0, 1, (n, 3)) * (_extent(c) + 8)
    s = rs.uniform(smin, smax, (n, 3))
    return np.hstack((rs.randint(0, B, (n, 1)), ctr - s / 2, ctr + s / 2)).tolist()


@functools.lru_cache(maxsize=None)
def rois(c):
    rs = np.random.RandomState(1000 + CASES.index(c))
    B = c.shape[0]
    if c.id == "shipped":
        rows = _classes(c, 0) + _classes(c, 1)
        rows += [[1, 10, 14, 6, 52, 40, 37]] * 3                                         # the same RoI three times
        rows += _random(c, rs, c.R - len(rows))
    elif c.id == "narrow_c":
        rows = [[0, -6, 10, -6, 40, 60, 30]]
    elif c.id == "table_edge":
        k = _classes(c, 0)
        rows = [k[0], k[2], k[11], k[12]]                                                # inside, x high face, whole map, z band
    elif c.id == "adaptive_tabled":
        # sizes in feature voxels (x, y, z) -> grid = ceil(size / 7); 63 is the largest the tables take
        rows = [[0, 8, -8, -20, 48, 88, 140],                                            # 5, 12, 20 -> grids 1, 2, 3: three axes differ
                [0, -200, -210, -220, 304, 294, 284],                                    # 63^3 -> 9, 9, 9
                [0, -60, 10, -100, 180, 74, 300],                                        # 30, 8, 50 -> 5, 2, 8
                [0, 20, 30, -6, 60, 70, 10],                                             # z band at grid 1
                [0, -6, -6, -6, 106, 50, 10],                                            # z band: 14, 7, 2 -> 2, 1, 1
                [0, 33, 34, 21, 35, 36, 23], [0, 40, 30, 20, 30, 50, 40],                # sub-voxel, malformed
                [0, 4000, 4000, 4000, 4000, 4000, 4000]]
        rows += _random(c, rs, 4, 30.0, 480.0)
    elif c.id == "adaptive_untabled":
        rows = [[0, -250, -260, -270, 390, 380, 370],                                    # 640 wide on all axes: grid 12, 12, 12
                [0, -200, 30, 20, 440, 70, 60],                                          # wide on x only: 12, 1, 1 - untabled as a whole
                [0, 16, 16, 16, 72, 64, 56],                                             # small, tabled: 1, 1, 1
                [0, 20, 30, -6, 100, 90, 50]]                                            # tabled: 2, 2, 1, z samples in the band
    elif c.id == "many_rois":
        k = _classes(c, 0)
        rows = k + [k[0]] * 6
        rows += _random(c, rs, c.R - len(rows), 1.0, 30.0)
    else:
        k = [r for b in range(B) for r in _classes(c, b)]
        keep = {"wide_c": (0, 13, 11, 8, 7), "avg_wrapper": (12, 0, 0, 7, 8, 9),
                "noncubic_a": (12, 26, 13, 7, 8, 9, 10, 11, 25), "noncubic_b": (12, 26, 13, 7, 8, 9, 10, 11, 25)}[c.id]
        rows = [k[i] for i in keep]
        rows += _random(c, rs, c.R - len(rows))
    out = np.array(rows, np.float64).astype(F32)
    assert out.shape == (c.R, 7), (c.id, out.shape)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def top(c):
    """seeded randn with a per-channel scale exp(randn), so that a channel mix-up shows; `shipped`: about 10 % exact zeros"""
    rs = np.random.RandomState(2000 + CASES.index(c))
    C = c.shape[1]
    t = rs.randn(c.R, C, *c.bins) * np.exp(rs.randn(1, C, 1, 1, 1))
    if c.id == "shipped":
        t[rs.uniform(0, 1, t.shape) < 0.1] = 0.0
    t = t.astype(F32)
    t.setflags(write=False)
    return t


# ---------------------------------------------------------------------------------------------- the fp32 sample tables
Axis = collections.namedtuple("Axis", "raw valid lo hi l h")       # arrays [A, grid]; raw: the coordinate before the <= 0 clamp
Geom = collections.namedtuple("Geom", "batch grid count axes")    # grid and axes in (z, y, x) order


def axis_table(start, bin_, grid, A, dim, limit, hi_is_lo=False):
    """make_sample of csrc/roi_align3d.hip for every (bin, sub-sample) of one axis, np.float32 arithmetic in its order"""
    p = np.arange(A, dtype=F32)[:, None]
    i = np.arange(grid, dtype=F32)[None, :]
    c = start + p * bin_
    c = c + (i + F32(.5)) * bin_ / F32(grid)
    assert c.dtype == F32
    raw = c
    valid = ~((raw.astype(np.float64) < limit) | (raw > F32(dim)))
    c = np.where(c <= 0, F32(0), c)
    lo = np.minimum(c, F32(2 ** 30)).astype(np.int64)
    at_end = lo >= dim - 1
    lo = np.where(at_end, dim - 1, lo)
    hi = np.where(at_end, dim - 1, lo + 1)
    c = np.where(at_end, lo.astype(F32), c)
    l = c - lo.astype(F32)
    h = (1.0 - l.astype(np.float64)).astype(F32)
    assert l.dtype == F32
    if hi_is_lo:
        hi = lo
    return Axis(raw, valid, lo, hi, l, h)


def roi_geometry(r, scale, bins, ratio, dims, z_limit=-0.1, hi_is_lo=False):
    """roi_geom + the three tables of one RoI row r (fp32 [7]); bins = (AS, AH, AW), dims = (S, H, W)"""
    scale = F32(scale)
    axes, grids = [], []
    for ax in range(3):                                     # z, y, x  <-  columns 3 / 6, 2 / 5, 1 / 4
        start = r[3 - ax] * scale
        end = r[6 - ax] * scale
        roi = np.maximum(end - start, F32(1))
        A = bins[ax]
        bin_ = roi / F32(A)
        grid = ratio if ratio > 0 else int(np.ceil(roi / F32(A)))
        assert isinstance(bin_, F32)
        grids.append(grid)
        axes.append(axis_table(start, bin_, grid, A, dims[ax], z_limit if ax == 0 else -1.0, hi_is_lo))
    return Geom(int(r[0]), tuple(grids), grids[0] * grids[1] * grids[2], tuple(axes))


def _matrices(t, A, dim):
    """M[p, d] = sum over the valid sub-samples of bin p of the weight on voxel d (fp64), N[p, d] = the number of adds behind it"""
    M, N = np.zeros((A, dim)), np.zeros((A, dim))
    p = np.broadcast_to(np.arange(A)[:, None], t.lo.shape)[t.valid]
    for idx, w in ((t.lo, t.h), (t.hi, t.l)):
        np.add.at(M, (p, idx[t.valid]), w[t.valid].astype(np.float64))
        np.add.at(N, (p, idx[t.valid]), 1.0)
    return M, N


Result = collections.namedtuple("Result", "grad A n geoms")


def reference(top_, rois_, shape, bins, scale, ratio, z_limit=-0.1, top_forward_order=False, count_plus=0, ignore_batch=False,
              hi_is_lo=False):
    """fp64 gradient [B, C, S, H, W] with A_e, n_e (module docstring) and the per-RoI tables.  The keyword arguments after `ratio` are the
    wrong backwards of the sensitivity test: the forward's z limit, the forward's (ph, pw, ps) order of `top`, count off by one, every RoI
    on batch item 0, both corners of an axis on the low voxel."""
    B, C, S, H, W = shape
    AS, AH, AW = bins
    R = rois_.shape[0]
    assert top_.shape == (R, C, AS, AH, AW) and rois_.shape == (R, 7)
    rois_ = np.asarray(rois_, F32)
    geoms = [roi_geometry(rois_[r], scale, bins, ratio, (S, H, W), z_limit, hi_is_lo) for r in range(R)]
    Mz, My, Mx = np.zeros((R, AS, S)), np.zeros((R, AH, H)), np.zeros((R, AW, W))
    n = np.zeros((B, 1, S, H, W))
    batch = np.zeros(R, np.int64)
    for r, g in enumerate(geoms):
        (Mz[r], nz), (My[r], ny), (Mx[r], nx) = (_matrices(t, A, d) for t, A, d in zip(g.axes, bins, (S, H, W)))
        Mz[r] /= float(g.count + count_plus)
        batch[r] = 0 if ignore_batch else g.batch
        assert 0 <= batch[r] < B
        n[batch[r], 0] += nz.sum(0)[:, None, None] * ny.sum(0)[None, :, None] * nx.sum(0)[None, None, :]
    t = np.asarray(top_, np.float64)
    if top_forward_order:                                   # the flat index the forward writes: (ph * AW + pw) * AS + ps
        t = t.reshape(R, C, AH, AW, AS).transpose(0, 1, 4, 2, 3)

    def push(t):
        a = np.einsum("rcijk,rkx->rcijx", t, Mx)
        a = np.einsum("rcijx,rjy->rciyx", a, My)
        a = np.einsum("rciyx,riz->rczyx", a, Mz)
        out = np.zeros((B, C, S, H, W))
        for b in range(B):
            out[b] = a[batch == b].sum(0)
        return out

    return Result(push(t), push(np.abs(t)), np.broadcast_to(n, (B, C, S, H, W)), geoms)


@functools.lru_cache(maxsize=None)
def reference_of(c):
    """the reference of a case of the table: computed once, shared, read-only"""
    res = reference(top(c), rois(c), c.shape, c.bins, c.scale, c.ratio)
    for a in (res.grad, res.A):
        a.setflags(write=False)
    return res


def bound(res):
    return (res.n + K_BOUND) * U * res.A


Verdict = collections.namedtuple("Verdict", "outside nonzero worst where")


def compare(got, res, extra_bound=None):
    """got [B, C, S, H, W] against a Result: the number of elements outside the bound, the number that are not 0.0 where A_e == 0, the
    largest |got - ref| / bound over the elements with A_e > 0 and its index (b, c, z, y, x)"""
    got = np.asarray(got, np.float64)
    assert got.shape == res.grad.shape, (got.shape, res.grad.shape)
    bd = bound(res) if extra_bound is None else bound(res) + extra_bound
    err = np.abs(got - res.grad)
    live = res.A > 0
    ratio = np.zeros_like(err)
    ratio[live] = err[live] / bd[live]
    where = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return Verdict(int((err > bd).sum()), int((got[~live] != 0.0).sum()), float(ratio[where]), tuple(int(i) for i in where))


def describe(v):
    return "%d elements outside the bound, %d not 0.0 where no add lands; largest err / bound %.4f at (b, c, z, y, x) = %s" % (
        v.outside, v.nonzero, v.worst, v.where)


# ---------------------------------------------------------------------------------------------- what launch() does with a case
def chunk_sizes(R, C):
    """channels per blockIdx.y of csrc/roi_align3d.hip launch(): C is cut while the grid has < 2048 workgroups and chunks stay >= 16"""
    chunks = 1
    while R * chunks < 2048 and chunks * 16 < C:
        chunks *= 2
    cpb = (C + chunks - 1) // chunks
    return [min(cpb, C - c0) for c0 in range(0, C, cpb)]


def untabled(g, bins):
    """the whole RoI takes roi_untabled_range as soon as one axis needs more than kMaxTable entries"""
    return any(A * grid > K_MAX_TABLE for A, grid in zip(bins, g.grid))
