"""The ordered RoIAlign3D backward (csrc/roi_align3d_bwd.hip; DESIGN.md, "RoIAlign3D backward, ordered"): its error bound, the extra
cases that reach its bucketing, partition and tiling, and a NumPy fp32 restatement of its operation order.  No tests live here:
tests/test_roi_align_backward_ordered_host.py and tests/test_gpu_roi_align_backward_ordered.py use it.  The semantics, the case table,
the fp64 reference (T.reference: grad, A_e, n_e) are those of tests/roi_align_backward_cases.py; nothing there is changed.

The kernel's operation order.  The table values (lo, hi, l, h, valid) are make_sample's, the same fp32 numbers as in the atomic kernel.
Per RoI r and axis, M[p, d] starts at 0 and takes, for the sub-samples i = 0 .. grid - 1 of bin p in order and only the valid ones,
M[p, lo] += h and then M[p, hi] += l (fp32).  With tq = fl(top[r, c, ps, ph, pw] / count), every sum starting at 0 and running in
ascending index,
    u[z, ph, pw] = sum_ps Mz[ps, z] * tq[ps, ph, pw]       (terms with Mz[ps, z] == 0 are skipped)
    v[z, y, pw]  = sum_ph My[ph, y] * u[z, ph, pw]
    w[z, y, x]   = sum_pw Mx[pw, x] * v[z, y, pw]
for the voxels of the box [zlo, zhi] x [ylo, yhi] x [xlo, xhi] that the RoI's valid samples reach per axis (a RoI with no valid sample on
an axis is skipped), one multiplication and one addition per step, no FMA.  The RoIs of image b, in ascending RoI index, form a list of
length L; wave k of nw = plan().nw takes its entries [k L // nw, (k + 1) L // nw) and adds each w, in list order, to its own zeroed copy
of the map: acc_k = acc_k + w.  The result is ((acc_0 + acc_1) + acc_2) + acc_3.  The map is cut into tiles of min(dim, 16) per axis; a
tile computes the part of each box inside it, which changes no value: every number above belongs to one voxel.

Error bound, per element e (derived, not fitted), with u = 2^-24 and n_e, A_e of T.reference:
    |got_e - ref_e| <= (n_e + K) * u * A_e,   K = 8,         and got_e == 0.0 exactly where A_e == 0.
Derivation.  A_e is the sum over the terms (r, ps, ph, pw) of |top| Mz My Mx / count.  To first order a term's relative error is u times
the number of roundings on its path:
    1            the division tq = fl(top / count) (count is a small integer, exact);
    Nz + Ny + Nx - 3   folding: M[p, d] is a sum of N[p, d] positive weights, the first add is to 0 and exact;
    3            the three multiplications;
    bz + by + bx - 3   the adds inside the three passes: b = the number of bins p with M[p, d] != 0 on the axis; the first add of a pass is to 0,
                 an add of a zero product is exact;
    R_e - 1      the adds across RoIs: on its wave's copy a term meets at most R_k - 1 later adds (R_k = the wave's RoIs that reach e),
                 then the copies of the other waves that reach e, at most R_e - R_k of them; adding a copy that is 0 at e is exact.
With n_axis = sum_p N[p, d] (the adds the atomic kernel makes on that axis at d) N + b - 2 <= n_axis - 1, because every other non-zero
bin holds at least one add.  So the path is at most 4 + (nz + ny + nx - 3) + (R_e - 1).  n_e = sum over the RoIs that reach e of
nz ny nx >= (R_e - 1) + nz ny nx of the term's own RoI, and for positive integers nz ny nx >= nz + ny + nx - 2, hence
nz + ny + nx - 3 <= n_e - (R_e - 1) - 1 and the path is at most n_e + 3: the first-order bound is (n_e + 3) u A_e, the atomic kernel's.
The remaining 5 of K = 8 are, as in roi_align_backward_cases.py, room for the second-order terms (n_e u relative to the first, a
worst case a measured error stays far inside) and the reference's fp64 roundings.  No product underflows: weights are zero or >= 2^-24,
|top| is zero or >= 4e-7, count <= 729, so the smallest non-zero w is above 1e-32.
A_e == 0 means every term at e has a zero factor; fp32 products and sums of zeros are zero (the sign of a zero does not count).

Largest |got - ref| / bound per case on the MI355X: DESIGN.md; tests/test_gpu_roi_align_backward_ordered.py prints them (pytest -s).
"""
import collections
import functools

import numpy as np

import roi_align_backward_cases as T

F32 = np.float32
K_BOUND = 8

# csrc/roi_align3d_bwd.hip: kTile, kMaxWaves, kLdsBudget, kTopStageMax
TILE, MAX_WAVES, LDS_BUDGET, TOP_STAGE_MAX = 16, 4, 65024, 1024

Plan = collections.namedtuple("Plan", "tile ntiles stage per_wave nw")


def plan(bins, dims):
    """make_plan of csrc/roi_align3d_bwd.hip: tile edges and tile counts (z, y, x), LDS floats per wave, waves per workgroup"""
    tile = tuple(min(d, TILE) for d in dims)
    ntiles = tuple((d + t - 1) // t for d, t in zip(dims, tile))
    nbins = bins[0] * bins[1] * bins[2]
    stage = nbins <= TOP_STAGE_MAX
    f = tile[0] * tile[1] * tile[2] + sum(a * t for a, t in zip(bins, tile)) + bins[1] * bins[2] + tile[1] * bins[2] + (nbins if stage else 0)
    per_wave = (f + 3) // 4 * 4
    return Plan(tile, ntiles, stage, per_wave, min(MAX_WAVES, LDS_BUDGET // (4 * per_wave)))


def shares(L, nw):
    """the list entries [i0, i1) of each wave"""
    return [(k * L // nw, (k + 1) * L // nw) for k in range(nw)]


# ---------------------------------------------------------------------------------------------- the extra cases
Case = T.Case
EXTRA = (
    # (i) larger than the 16^3 tile on every axis and no multiple of it: 2 x 2 x 3 tiles, nw = 3
    Case("tiled", (1, 3, 19, 21, 37), (7, 7, 7), 2, 13, 0.125),
    # (ii) B = 3, no RoI on image 1
    Case("empty_middle", (3, 3, 6, 9, 11), (7, 7, 7), 2, 11, 0.125),
    # (iii) every RoI on the last image
    Case("last_image", (2, 3, 6, 9, 11), (3, 3, 3), 2, 7, 0.125),
    # (iv) nw = 4: image 0 has 2 RoIs (fewer than waves), image 1 has 7 (no multiple)
    Case("short_lists", (2, 4, 6, 9, 11), (7, 7, 7), 2, 9, 0.125),
    # (v) no RoI at all
    Case("no_rois", (2, 2, 4, 5, 6), (7, 7, 7), 2, 0, 0.125),
)
EXTRA_BY_ID = {c.id: c for c in EXTRA}
ACCEPTED = tuple(c for c in T.CASES if c.id != "adaptive_untabled")        # the ordered path refuses an adaptive grid beyond the tables


@functools.lru_cache(maxsize=None)
def rois(c):
    if c in T.CASES:
        return T.rois(c)
    rs = np.random.RandomState(5000 + EXTRA.index(c))
    if c.id == "tiled":
        # feature voxels = image voxels / 8; the map is 37 x 21 x 19 (x, y, z), tile borders at 16 and 32 on x, 16 on y and z
        rows = [[0, -10, -10, -10, 310, 180, 165],                         # covers all 12 tiles
                [0, 8, 8, 8, 100, 100, 100],                               # inside tile (0, 0, 0): feature voxels 1 .. 12.5
                [0, 100, 20, 20, 160, 90, 90],                             # straddles x = 16 only
                [0, 20, 100, 20, 90, 160, 90],                             # straddles y = 16
                [0, 20, 20, 100, 90, 90, 150],                             # straddles z = 16
                [0, 90, 90, 90, 290, 165, 150],                            # straddles all borders, both x borders
                [0, 264, 136, 136, 292, 164, 148]]                         # inside the last tile (x >= 32, y >= 16, z >= 16)
        rows += T._random(c, rs, c.R - len(rows), 8.0, 120.0)
    elif c.id == "empty_middle":
        rows = T._classes(c, 0)[:4] + T._classes(c, 2)[:3]
        more = T._random(c, rs, c.R - len(rows))
        for i, r in enumerate(more):
            r[0] = (0, 2)[i % 2]
        rows += more
    elif c.id == "last_image":
        rows = T._classes(c, 1)[:3] + T._random(c, rs, c.R - 3)
        for r in rows:
            r[0] = 1
    elif c.id == "short_lists":
        rows = T._random(c, rs, c.R)
        for i, r in enumerate(rows):
            r[0] = 0 if i in (3, 6) else 1                                 # interleaved: the lists are a compaction, not a prefix
    else:
        rows = []
    out = np.array(rows, np.float64).astype(F32).reshape(-1, 7)
    assert out.shape == (c.R, 7), (c.id, out.shape)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def top(c):
    if c in T.CASES:
        return T.top(c)
    rs = np.random.RandomState(6000 + EXTRA.index(c))
    C = c.shape[1]
    t = (rs.randn(c.R, C, *c.bins) * np.exp(rs.randn(1, C, 1, 1, 1))).astype(F32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def reference_of(c):
    if c in T.CASES:
        return T.reference_of(c)
    res = T.reference(top(c), rois(c), c.shape, c.bins, c.scale, c.ratio)
    for a in (res.grad, res.A):
        a.setflags(write=False)
    return res


def compare(got, res):
    """T.compare with this module's K"""
    return T.compare(got, res, extra_bound=(K_BOUND - T.K_BOUND) * T.U * res.A if K_BOUND != T.K_BOUND else None)


# ---------------------------------------------------------------------------------------------- the kernel's order in NumPy fp32
def fold(t, A, dim):
    """M[p, d] of one axis in the kernel's order (fp32): sub-samples in order, h to lo and then l to hi"""
    M = np.zeros((A, dim), F32)
    p = np.arange(A)
    for i in range(t.lo.shape[1]):
        ok = t.valid[:, i]
        M[p[ok], t.lo[ok, i]] = M[p[ok], t.lo[ok, i]] + t.h[ok, i]
        M[p[ok], t.hi[ok, i]] = M[p[ok], t.hi[ok, i]] + t.l[ok, i]
    assert M.dtype == F32
    return M


def reach(t):
    """[lo, hi] voxel range of the valid samples of one axis, or None"""
    if not t.valid.any():
        return None
    return int(t.lo[t.valid].min()), int(t.hi[t.valid].max())


def roi_term(top_r, g, bins, dims):
    """w [C, box] of one RoI and its box (slices), or None when an axis has no valid sample"""
    rng = [reach(t) for t in g.axes]
    if any(r is None for r in rng):
        return None
    (z0, z1), (y0, y1), (x0, x1) = rng
    Mz, My, Mx = (fold(t, A, d) for t, A, d in zip(g.axes, bins, dims))
    Mz, My, Mx = Mz[:, z0:z1 + 1], My[:, y0:y1 + 1], Mx[:, x0:x1 + 1]
    tq = top_r / F32(g.count)                                       # [C, AS, AH, AW]
    assert tq.dtype == F32
    C = top_r.shape[0]
    u = np.zeros((C, Mz.shape[1], bins[1], bins[2]), F32)
    for ps in range(bins[0]):
        m = Mz[ps][None, :, None, None]
        u = np.where(m == 0, u, u + m * tq[:, ps][:, None, :, :])
    v = np.zeros((C, Mz.shape[1], My.shape[1], bins[2]), F32)
    for ph in range(bins[1]):
        v = v + My[ph][None, None, :, None] * u[:, :, ph][:, :, None, :]
    w = np.zeros((C, Mz.shape[1], My.shape[1], Mx.shape[1]), F32)
    for pw in range(bins[2]):
        w = w + Mx[pw][None, None, None, :] * v[:, :, :, pw][:, :, :, None]
    assert w.dtype == F32
    return w, (slice(z0, z1 + 1), slice(y0, y1 + 1), slice(x0, x1 + 1))


def image_lists(geoms, B, order=None):
    """the RoIs of each image in ascending RoI index (order: another sequence of all RoI indices, for the order test)"""
    idx = range(len(geoms)) if order is None else order
    return [[r for r in idx if geoms[r].batch == b] for b in range(B)]


def ordered_backward(top_, rois_, shape, bins, scale, ratio, order=None):
    """the gradient [B, C, S, H, W] in fp32, operation for operation as the kernel computes it"""
    B, C, S, H, W = shape
    dims = (S, H, W)
    rois_ = np.asarray(rois_, F32).reshape(-1, 7)
    geoms = [T.roi_geometry(rois_[r], scale, bins, ratio, dims) for r in range(rois_.shape[0])]
    assert not any(T.untabled(g, bins) for g in geoms), "the ordered backward refuses this call"
    nw = plan(bins, dims).nw
    out = np.zeros(shape, F32)
    for b, lst in enumerate(image_lists(geoms, B, order)):
        copies = np.zeros((nw, C, S, H, W), F32)
        for k, (i0, i1) in enumerate(shares(len(lst), nw)):
            for r in lst[i0:i1]:
                term = roi_term(np.asarray(top_[r], F32), geoms[r], bins, dims)
                if term is None:
                    continue
                w, (sz, sy, sx) = term
                copies[k][:, sz, sy, sx] = copies[k][:, sz, sy, sx] + w
        acc = copies[0]
        for k in range(1, nw):
            acc = acc + copies[k]
        out[b] = acc
    assert out.dtype == F32
    return out
