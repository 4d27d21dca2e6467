"""Case tables, inputs, fp64 references, bounds and a NumPy emulation of both small-window GEMMs of the peak back-propagation:
csrc/prm_small_f16.hip (m3d_prm_small_dgrad_f16, the f16x2 split: the default of ops.SmallWindowDgrad wherever the forward conv's cout
is a multiple of 16) and csrc/prm_small.hip (m3d_prm_small_dgrad, the fp32 MFMA form).  No tests live here:
tests/test_prm_small_cases_host.py proves on the CPU that the tables reach what they claim, that the exact operands are exact, that the
emulation of the unmutated launch equals the fp64 reference and fits every bound, and that the exact comparison catches every seeded
defect; tests/test_gpu_prm_small.py runs the tables on the GPU.

Operation (tests/prm_stage_cases.py: ref_dgrad, written on whole maps, none of the kernels' index arithmetic):
    out[p, co, v] = (X[co][origin_p + v] - off) * sum_{ci, t} relu(W)[ci][co][26 - t] G_N[p, ci][v + t - 1],   0 outside the map.
A case is (win, cg = cout_fwd = channels of G_N, cx = cin_fwd = channels of X and of the output, P).

Geometry mirrored from the two .hip files (`geom`): columns n = p V + v flattened densely over the batch, V = win^3; a workgroup owns
`cols` consecutive columns (f16: 128 for win 3, 256 for 5 and 7; fp32: 128) x 32 output channels and stages the windows of
PK = (cols - 1) / V + 2 peak slots (f16 6 / 4 / 2, fp32 6 / 3 / 2), slot s = peak (n0 / V) + s, with a one-voxel zero border;
K runs in chunks of CK input channels (f16 16 = one MFMA, lane half h = 8 channels; fp32 4, the last chunk ragged).

Comparisons (u = 2^-24):
 (a) exact: G_N integers in [-3, 3] (f16 table: peak p times 2^k_p, k_p spread over [-20, 20]; the per-peak scale is a power of two),
     W integers in [-2, 2], X - off integers in [-2, 3], Cabs < 2^24 in the peak's own units: every summation order is exact, the
     result EQUALS the fp64 reference bit for bit (the sign of a zero is not compared).
 (b) lo-plane probes (f16): the integers of (a) never fill the low fp16 piece.  Two sparse sets per window size (PROBE_SHAPES):
     "gn": one non-zero G_N element per peak, an odd 22-bit integer times 2^k_p, W in [-2, 2]: every output is ONE product;
     "w":  one weight is an odd 22-bit integer, the others in [-2, 2], G_N in [-3, 3] 2^k_p, X - off a power of two or 0: a sum with
           no rounding (Cabs of the cut pieces < 2^24).
     The probes move over both lane halves (channels 8 h + j), both chunk parities and the first, interior and last tap; that the cut
     loses nothing (l_a l_b == 0 everywhere) is computed with f16x2_contract.cut, not assumed.
 (c) bounded: the input families of f16x2_contract.inputs, per-peak magnitudes spread over 2^-24 .. 2^24.
     f16:  the contract's E (f16x2_contract.bound("prm_small", cg, ...)) with gain = |X - off|, A = max |G_N[p]|, B = max relu(W);
     fp32: prm_stage_cases.bound_sum(y, Cabs |X - off|, 27 cg), as test_dgrad_prehook uses.
     Exact zeros where C == 0 and outside the map.
 (d) clamp edge (f16): f16_scale_of clamps the scale at 2^125, so a peak with A = max |G_N[p]| < 2^-111 is scaled by less than the
     contract assumes (1 / s <= A 2^-14).  With the clamp 1 / s = 2^-125 = A_eff 2^-14 for A_eff = max(A, 2^-111): every step of the
     contract's derivation holds with A_eff in place of A (|a| <= A <= A_eff), so the bound of such a peak is E evaluated at A_eff.
     CLAMP_CASE holds peaks with A = 2^-100 (not clamped), 2^-112, 2^-125 and an all-zero peak among ordinary ones.  Outputs of the
     smallest peak reach below 2^-126, where an fp32 result rounds to a multiple of 2^-149: an absolute error the contract's relative
     last term (u |y|) does not contain.  The batch keeps |X - off| >= 1 where the window is inside the map and the host test asserts that the
     cut's own absolute term of E at A_eff (gain 1.001 2^-150 sum |b|) is at least the three such roundings of the epilogue
     ((1 + gain) 2^-150): nothing is added to E.

Emulation (`emulate`): one launch of either kernel from the documented geometry - pack image in the kernel's lane order, column ->
(peak, voxel), slot table of a workgroup, chunk loop (f16: tot += acc after every second chunk and after the last; fp32: 4-channel
chunks with a ragged tail), tap flip 26 - t, PreHook multiply at origin + v, zero outside the map, un-scaling with the column's own
peak.  Sums are fp64 (no accumulation error); the epilogue's multiplies are fp32.  `defect` seeds one of DEFECTS.

Largest measured |got - y| / bound (MI355X, printed by tests/test_gpu_prm_small.py with pytest -s; documentation of the margin, no
threshold is set from them; every exact comparison held bit for bit):
    f16x2 split   win 3: 0.0931   win 5: 0.2036 (quiet)   win 7: 0.0760   clamp edge: 0.0087 (2^-100 0.0087, 2^-112 0.0079, 2^-125 0.0053)
    fp32 MFMA     win 3: 0.0143   win 5: 0.0357           win 7: 0.0042
"""
import collections
import functools
import zlib

import numpy as np
import torch

import f16x2_contract as K
import prm_stage_cases as T

F32, F64 = np.float32, np.float64
LIMIT = 2.0 ** 24

# ------------------------------------------------------------------ constants of the two kernels, mirrored once
Geom = collections.namedtuple("Geom", "kind win V PW CSB cols PK CK")


def geom(kind, win):
    """prm_small_f16.hip: kC16 = 16, WAVES = 4 (win 3) / 8 (5, 7), kCols = 32 WAVES, PK = (kCols - 1) / V + 2;
    prm_small.hip: kCC = 4, 128 columns, PK = 127 / V + 2"""
    assert kind in ("f16", "f32") and win in (3, 5, 7)
    V = win ** 3
    cols = 128 if (kind == "f32" or win == 3) else 256
    return Geom(kind, win, V, win + 2, (win + 2) ** 3, cols, (cols - 1) // V + 2, 16 if kind == "f16" else 4)


F16_MAX_PEAKS = 65535                  # m3d_prm_small_dgrad_f16 refuses more per launch

SmallCase = collections.namedtuple("SmallCase", "win cg cx P")
F16_CASES = (
    SmallCase(3, 16, 24, 1),       # one chunk: the only flush is ch + 1 == nchunk on an even ch; 27 of 128 columns; cx below a block
    SmallCase(3, 48, 33, 24),      # three chunks: a flush after chunk 1, the lone chunk 2 flushed by the end rule; the second block holds one
                                   # channel; workgroup 4 starts at voxel 26 of peak 18 and uses all 6 slots; the last has 8 columns and
                                   # slots for peaks that do not exist
    SmallCase(3, 256, 64, 19),     # 16 chunks (the RPN conv's K); 513 columns = 4 workgroups + 1 column
    SmallCase(5, 32, 40, 44),      # the <5, 8> instance; workgroup 20 starts at voxel 120 and uses all 4 slots
    SmallCase(5, 80, 96, 3),       # five chunks; three output-channel blocks
    SmallCase(7, 16, 32, 1),       # 343 columns = 1 workgroup + 87; exactly one block
    SmallCase(7, 64, 33, 4),       # both slots; 4 chunks
    SmallCase(7, 256, 24, 2),      # the production K at the widest window
)
F32_CASES = (
    SmallCase(3, 1, 5, 1),         # one channel: three of the chunk's four channel rows empty
    SmallCase(3, 64, 33, 24),      # 16 chunks; slot 6 used
    SmallCase(3, 12, 40, 128),     # 3456 columns = exactly 27 workgroups, no partial one
    SmallCase(5, 8, 40, 44),       # workgroup 41 uses all 3 slots
    SmallCase(5, 130, 24, 3),      # 33 chunks, the last with 2 channels
    SmallCase(7, 256, 64, 2),      # the production shape
)
CASES = {"f16": F16_CASES, "f32": F32_CASES}
PROBE_SHAPES = {3: SmallCase(3, 48, 33, 12), 5: SmallCase(5, 48, 33, 6), 7: SmallCase(7, 48, 33, 4)}
PROBES = ("gn", "w")
# the big weight of the "w" probe (ci, co, tz, ty, tx): win 3 the first tap, lane half 1 of the odd chunk, the ragged second block's one
# channel; win 5 an interior tap, half 0 of chunk 0; win 7 the last tap, half 1 of the even chunk 2
PROBE_W_AT = {3: (16 + 11, 32, 0, 0, 0), 5: (4, 7, 1, 2, 0), 7: (32 + 9, 20, 2, 2, 2)}
FAMILIES = ("benign", "heavy", "outlier12", "outlier24", "outlier36", "quiet", "at_bound_pow2", "at_bound_below", "zero")
# the cases that get every family (f16) / benign, heavy and zero (fp32); every other case: benign
F16_ALL_FAMILIES = (SmallCase(3, 48, 33, 24), SmallCase(5, 32, 40, 44), SmallCase(7, 64, 33, 4))
F32_FAMILIES = ("benign", "heavy", "zero")
F32_ALL_FAMILIES = (SmallCase(3, 64, 33, 24), SmallCase(5, 8, 40, 44), SmallCase(7, 256, 64, 2))
CLAMP_CASE = SmallCase(3, 32, 33, 9)
CLAMP_PEAKS = {2: -100, 4: -112, 6: -125}          # peak: log2 of its max |G_N|
CLAMP_ZERO_PEAK = 7
A_EFF_MIN = 2.0 ** -111


def bounded_table(kind):
    """[(case, family)] of the bounded comparison"""
    allf, fams = (F16_ALL_FAMILIES, FAMILIES) if kind == "f16" else (F32_ALL_FAMILIES, F32_FAMILIES)
    return [(c, f) for c in CASES[kind] for f in (fams if c in allf else ("benign",))]


def case_id(c):
    return "w%d-%dto%d-p%d" % tuple(c)


def map_shape(c):
    return (5, 6, 7) if c.win == 3 else (9, 11, 13)


def _seed(c, salt):
    return zlib.crc32(repr(tuple(c)).encode()) + salt


def workgroups(kind, c):
    """per workgroup of the launch: (n0, first peak, valid columns, slots its columns use, slots that name a peak >= P)"""
    g = geom(kind, c.win)
    ntot = c.P * g.V
    out = []
    for n0 in range(0, ntot, g.cols):
        ncol = min(g.cols, ntot - n0)
        p_first = n0 // g.V
        used = (n0 + ncol - 1) // g.V - p_first + 1
        out.append((n0, p_first, ncol, used, max(0, p_first + g.PK - c.P)))
    return out


def nchunk(kind, c):
    return -(-c.cg // geom(kind, c.win).CK)


# ------------------------------------------------------------------ inputs
def origins(c, rng):
    """seeded over [-win - 1, extent + 2) (three of four peaks then clipped to where the window still reaches the map, so that a
    workgroup's later slots hold windows whose outputs are not all zero); peak 0 at (-1, -2, -1); P >= 3: peak 2 wholly outside"""
    D, H, W = map_shape(c)
    o = np.stack([rng.integers(-c.win - 1, e + 2, c.P) for e in (D, H, W)], 1).astype(np.int32)
    keep = np.arange(c.P) % 4 == 3                                      # every fourth peak stays as drawn (it may miss the map) ..
    reach = np.stack([np.clip(o[:, a], 1 - c.win, e - 1) for a, e in enumerate((D, H, W))], 1)
    o = np.where(keep[:, None], o, reach).astype(np.int32)              # .. the others are moved until one voxel is inside
    o[0] = (-1, -2, -1)
    if c.P >= 3:
        o[2] = T.origins_for("out", (D, H, W), c.win)[1]
    return o


def peak_exponents(P, rng):
    """k_p spread over [-20, 20], in a seeded order (neighbouring peaks - one workgroup - get different scales)"""
    k = np.round(np.linspace(-20, 20, P)).astype(np.int64) if P > 1 else np.array([-13])
    return rng.permutation(k)


def exact_inputs(kind, c):
    rng = np.random.default_rng(_seed(c, 71 if kind == "f16" else 72))
    gn = rng.integers(-3, 4, (c.P, c.cg) + (c.win,) * 3).astype(F32)
    gn[:, 0, 0, 0, 0] = 3                                               # every peak's max |G_N| is 3 2^k_p
    kp = np.zeros(c.P, np.int64)
    if kind == "f16":
        kp = peak_exponents(c.P, rng)
        gn = gn * (2.0 ** kp).astype(F32).reshape(-1, 1, 1, 1, 1)
    w = rng.integers(-2, 3, (c.cg, c.cx, 3, 3, 3)).astype(F32)
    full = rng.integers(-1, 5, (c.cx,) + map_shape(c)).astype(F32)
    return dict(gn=gn, w=w, full=full, off=F32(1.0), origin=origins(c, rng), kp=kp)


def odd22(rng):
    return float(2 * int(rng.integers(2 ** 20, 2 ** 21)) + 1)          # an odd integer in [2^21, 2^22): 22 significant bits


def probe_positions(c):
    """(channel, voxel) of peak p's probe: channels walk over both lane halves and every chunk, voxels over corner, centre, last"""
    V = c.win ** 3
    chans = [(5 * p + 16 * (p // 2) + 8 * (p % 2)) % c.cg for p in range(c.P)]
    vox = [(0, V // 2, V - 1, 1 + p)[p % 4] % V for p in range(c.P)]
    return chans, vox


def probe_inputs(win, which):
    c = PROBE_SHAPES[win]
    rng = np.random.default_rng(_seed(c, 81 if which == "gn" else 82))
    kp = peak_exponents(c.P, rng)
    w = rng.integers(-2, 3, (c.cg, c.cx, 3, 3, 3)).astype(F32)
    o = origins(c, rng)
    o[1] = (0, 1, 0)                                                    # one window wholly inside the map
    if which == "gn":
        gn = np.zeros((c.P, c.cg, c.win ** 3), F32)
        chans, vox = probe_positions(c)
        for p in range(c.P):
            gn[p, chans[p], vox[p]] = odd22(rng) * (-1) ** p
        gn = gn.reshape((c.P, c.cg) + (c.win,) * 3)
        full = rng.integers(-1, 5, (c.cx,) + map_shape(c)).astype(F32)          # X - off in -2 .. 3: 22 bits x 3 fits 24
    else:
        gn = rng.integers(-3, 4, (c.P, c.cg) + (c.win,) * 3).astype(F32)
        gn[:, 0, 0, 0, 0] = 3
        w[PROBE_W_AT[win]] = odd22(rng)
        full = rng.choice(np.array([-1.0, 0.0, 1.0, 2.0, 3.0, 5.0], F32), (c.cx,) + map_shape(c))      # X - off in {-2, -1, 0, 1, 2, 4}
    gn = gn * (2.0 ** kp).astype(F32).reshape(-1, 1, 1, 1, 1)
    return dict(gn=gn, w=w, full=full, off=F32(1.0), origin=o, kp=kp)


def bounded_inputs(kind, c, family):
    seed = _seed(c, 91 if kind == "f16" else 92) % (2 ** 31)
    gn, w = K.inputs(family, (c.P, c.cg) + (c.win,) * 3, (c.cg, c.cx, 3, 3, 3), seed, signed=True)
    if family != "zero" and not family.startswith("at_bound"):
        gn = gn * (2.0 ** torch.linspace(-24, 24, c.P)).view(c.P, 1, 1, 1, 1)   # each peak starts from its own (1 - y) y
    rng = np.random.default_rng(seed)
    full = rng.standard_normal((c.cx,) + map_shape(c)).astype(F32)
    return dict(gn=gn.numpy().astype(F32), w=w.numpy().astype(F32), full=full, off=full.min(), origin=origins(c, rng))


def clamp_inputs():
    c = CLAMP_CASE
    e = bounded_inputs("f16", c, "benign")
    gn = e["gn"]
    for p, k in CLAMP_PEAKS.items():
        gn[p] = (gn[p] / np.abs(gn[p]).max()).astype(F32) * F32(2.0 ** k)       # max |G_N[p]| is exactly 2^k (x / x == 1)
        assert np.abs(gn[p]).max() == F32(2.0 ** k)
    gn[CLAMP_ZERO_PEAK] = 0
    rng = np.random.default_rng(7)
    full = rng.uniform(1.0, 4.0, e["full"].shape).astype(F32)                    # off = 0: |X - off| >= 1 (the docstring's (d))
    o = e["origin"]
    for p in CLAMP_PEAKS:
        o[p] = (p % 3 - 1, 1, p % 2)                                             # the tiny peaks reach the map
    return dict(gn=gn, w=e["w"], full=full, off=F32(0.0), origin=o)


# ------------------------------------------------------------------ references and bounds
def reference(e):
    """(y, Cabs |X - off|) in fp64"""
    return T.ref_dgrad(e["gn"], e["w"], e["full"], e["off"], e["origin"], want_cabs=True)


def multiplier(e):
    """(X[origin + v] - off in fp64 [P, cx, n, n, n], inside-the-map mask)"""
    n = e["gn"].shape[2]
    m = np.stack([T.crop(e["full"].astype(F64) - F64(e["off"]), o, n) for o in e["origin"]])
    inmap = np.stack([T.crop(np.ones(e["full"].shape, bool), o, n) for o in e["origin"]])
    return m, inmap


def f16_terms(e):
    gn, wr = torch.from_numpy(e["gn"]), torch.relu(torch.from_numpy(e["w"]))
    return K.terms(K.dgrad_op, gn, wr)


def f16_bound(e, y, a_eff=False):
    """(E, live): the contract's E of every output with gain |X - off| (0 outside the map), A per peak (a_eff: max(A, 2^-111)), and
    live = the outputs that are not exact zeros (C > 0 inside the map)"""
    gn, wr = torch.from_numpy(e["gn"]), torch.relu(torch.from_numpy(e["w"]))
    C, Sa, Sb, n = K.terms(K.dgrad_op, gn, wr)
    A = gn.abs().amax(dim=(1, 2, 3, 4)).to(torch.float64).view(-1, 1, 1, 1, 1)
    if a_eff:
        A = A.clamp_min(A_EFF_MIN)
    m, inmap = multiplier(e)
    E = K.bound("prm_small", e["gn"].shape[1], C, Sa, Sb, n, A, float(wr.max()), torch.from_numpy(y), gain=torch.from_numpy(np.abs(m)))
    return E.numpy(), inmap & (C.numpy() > 0)


def f32_bound(e, y, cabs):
    return T.bound_sum(y, cabs, 27 * e["gn"].shape[1]), cabs > 0


@functools.lru_cache(maxsize=None)
def exact_reference(kind, c):
    e = exact_inputs(kind, c)
    return (e,) + reference(e)


@functools.lru_cache(maxsize=None)
def probe_reference(win, which):
    e = probe_inputs(win, which)
    return (e,) + reference(e)


@functools.lru_cache(maxsize=None)
def bounded_reference(kind, c, family):
    """(inputs, y, bound, live) - computed once per process, left unchanged by the tests that share it"""
    e = bounded_inputs(kind, c, family)
    y, cabs = reference(e)
    return (e, y) + (f16_bound(e, y) if kind == "f16" else f32_bound(e, y, cabs))


@functools.lru_cache(maxsize=None)
def clamp_reference():
    e = clamp_inputs()
    y, _ = reference(e)
    return (e, y) + f16_bound(e, y, a_eff=True)


def held(got, y, bound, live, what):
    """worst |got - y| / bound; every output finite, exact zeros where nothing is summed (C == 0) and outside the map"""
    got = np.asarray(got)
    assert np.all(np.isfinite(got)), what + ": not finite"
    assert not np.any(got[~live]), what + ": %d non-zero outputs where C == 0 or outside the map" % int(np.count_nonzero(got[~live]))
    return T.ratio(got, y, bound, what, signs=False)


# ------------------------------------------------------------------ the emulation of one launch
DEFECTS = {          # name: the kinds it exists in
    "tap_not_flipped": ("f16", "f32"),          # pack reads W[..][t] in place of W[..][26 - t]
    "roles_swapped": ("f16", "f32"),            # pack indexes W as [cin_fwd][cout_fwd][27]
    "flush_skipped_even_last": ("f16",),        # the flush rule is (ch & 1) alone: the lone last chunk of an odd count never reaches tot
    "flush_every_chunk": ("f16",),              # tot += acc after every chunk, acc restarted by the rule only: a chunk counted twice
    "unscale_first_peak": ("f16",),             # inv_p of the workgroup's first peak
    "slot_short": ("f16", "f32"),               # slot index p - p_first - 1 (floor 0) in workgroups that start mid-peak
    "border_neighbour": ("f16", "f32"),         # the one-voxel border of a slot holds the next slot's window, wrapped, instead of zero
    "lo_half": ("f16",),                        # the lo plane of lane half 1 read at half 0's unit
    "drop_hilo": ("f16",),                      # no hi(W) lo(G_N) product
    "drop_lohi": ("f16",),                      # no lo(W) hi(G_N) product
    "mult_no_v": ("f16", "f32"),                # X read at origin, not origin + v
    "clamped_read": ("f16", "f32"),             # outside the map: the clamped voxel's value in place of 0
    "fold_store": ("f16", "f32"),               # a ragged block's channels >= cx stored to channel co % cx
    "partial_dropped": ("f16", "f32"),          # grid = ntot / cols rounded down
    "ragged_runs_on": ("f32",),                 # the ragged chunk's rows >= cg neither masked in the pack (channel folded) nor in the
}                                               # staging: they read on into the next peak's channel 0 ..


def applies(defect, kind, c, probe=None):
    """whether the exact comparison of this case must catch the defect (from the geometry alone).  Probe sets (sparse data) are asked
    only for the three defects that need a filled lo plane; the tables' integers never fill it."""
    if kind not in DEFECTS[defect]:
        return False
    lo = {"lo_half": "gn", "drop_hilo": "gn", "drop_lohi": "w"}
    if probe is not None or defect in lo:
        return probe is not None and lo.get(defect) == probe
    g, wgs, nch = geom(kind, c.win), workgroups(kind, c), nchunk(kind, c)
    e = exact_reference(kind, c)[0]
    col_in = multiplier(e)[1][:, 0].reshape(-1)                         # column n = p V + v lies inside the map
    col_p = np.arange(c.P * g.V) // g.V

    def later(n0, p_first, ncol, other_scale=False):
        """a column of the workgroup inside the map whose peak is not the workgroup's first (and is scaled differently)"""
        sel = col_in[n0:n0 + ncol] & (col_p[n0:n0 + ncol] > p_first)
        if other_scale:
            sel = sel & (e["kp"][col_p[n0:n0 + ncol]] != e["kp"][p_first])
        return bool(sel.any())

    return {
        "tap_not_flipped": True,
        "roles_swapped": c.cg > 1 and c.cx > 1,
        "flush_skipped_even_last": nch % 2 == 1,
        "flush_every_chunk": nch >= 2,
        "unscale_first_peak": any(later(n0, pf, ncol, True) for n0, pf, ncol, _, _ in wgs),
        "slot_short": any(n0 % g.V and later(n0, pf, ncol) for n0, pf, ncol, _, _ in wgs),
        "border_neighbour": c.P >= 2,
        "mult_no_v": True,
        "clamped_read": True,
        "fold_store": c.cx % 32 != 0,
        "partial_dropped": (c.P * g.V) % g.cols != 0,
        "ragged_runs_on": c.cg % 4 != 0 and c.P >= 2,
    }[defect]


def _padded(win, nb=None):
    """win [..., n, n, n] with the one-voxel border: zero, or (nb given: defect border_neighbour) nb wrapped around"""
    pad = [(0, 0)] * (win.ndim - 3) + [(1, 1)] * 3
    out = np.pad(win, pad)
    if nb is not None:
        n = win.shape[-1]
        border = np.ones((n + 2,) * 3, bool)
        border[1:-1, 1:-1, 1:-1] = False
        out[..., border] = np.pad(nb, pad, mode="wrap")[..., border]
    return out


def _cut(a, bound):
    h, l = K.cut(torch.from_numpy(np.ascontiguousarray(a, F32)), torch.from_numpy(np.asarray(bound, F32)))
    return h.numpy(), l.numpy()


def pack_image(kind, w, defect=None):
    """relu(W) in the kernels' packed order.  f16: (hi, lo) [cb][chunk][tap][lane][j], unscaled fp64, ci = 16 chunk + 8 (lane >> 5) + j;
    fp32: [cb][chunk][cp][tap quad][lane][tap % 4], ci = 4 chunk + 2 cp + (lane >> 5); co = 32 cb + (lane & 31) in both"""
    cg, cx = w.shape[:2]
    wr = np.maximum(w.reshape(cg, cx, 27), 0).astype(F32)
    ncb = (cx + 31) // 32
    lane = np.arange(64)
    co = (32 * np.arange(ncb)[:, None] + (lane & 31)[None, :])                  # [cb, lane]
    if kind == "f16":
        nch = cg // 16
        ci = 16 * np.arange(nch)[:, None, None] + 8 * (lane >> 5)[None, :, None] + np.arange(8)      # [chunk, lane, j]
        t = np.arange(27)
        CO, CI, TT = co[:, None, None, :, None], ci[None, :, None, :, :], t[None, None, :, None, None]
        ok = (CO < cx) & (CI < cg) & (TT < 27)
    else:
        nch = -(-cg // 4)
        ci = 4 * np.arange(nch)[:, None, None] + 2 * np.arange(2)[None, :, None] + (lane >> 5)       # [chunk, cp, lane]
        t = 4 * np.arange(7)[:, None] + np.arange(4)                                                  # [tq, tj]
        CO, CI, TT = co[:, None, None, None, :, None], ci[None, :, :, None, :, None], t[None, None, None, :, None, :]
        ok = (CO < cx) & (TT < 27)
        if defect == "ragged_runs_on":
            CI = CI % cg
        ok = ok & (CI < cg)
    tt = TT if defect == "tap_not_flipped" else 26 - TT
    idx = ((CO * cg + CI) if defect == "roles_swapped" else (CI * cx + CO)) * 27 + tt
    idx = np.where(ok, idx, 0)
    if kind == "f32":
        return np.where(ok, wr.reshape(-1).astype(F64)[idx], 0.0)
    wh, wl = _cut(wr, wr.max())
    return np.where(ok, wh.reshape(-1)[idx], 0.0), np.where(ok, wl.reshape(-1)[idx], 0.0)


def emulate(kind, gn, w, full, off, origin, defect=None):
    """out [P, cx, n, n, n] fp32 of one launch (NaN where the launch writes nothing)"""
    assert defect is None or kind in DEFECTS[defect], (kind, defect)
    P, cg, win = gn.shape[:3]
    cx = w.shape[1]
    g = geom(kind, win)
    V, PW, CSB, PK, CK = g.V, g.PW, g.CSB, g.PK, g.CK
    nch, ncb = -(-cg // CK), (cx + 31) // 32
    D, H, Wd = full.shape[1:]
    f16 = kind == "f16"
    if f16:
        assert cg % 16 == 0 and P <= F16_MAX_PEAKS
        amax = np.abs(gn).reshape(P, -1).max(1)
        gh, gl = _cut(gn, amax.reshape(P, 1, 1, 1, 1))
        sp = np.array([K.scale_of(a)[0] for a in amax])
        sw = K.scale_of(np.maximum(w, 0).max())[0]
        ah_all, al_all = pack_image(kind, w, defect)
    else:
        a_all = pack_image(kind, w, defect)
    gflat = gn.reshape(-1).astype(F64)
    out = np.full((P, cx, V), np.nan, F32)
    ntot = P * V
    nwg = ntot // g.cols if defect == "partial_dropped" else -(-ntot // g.cols)
    t = np.arange(27)
    toff = ((t // 9) * PW + (t // 3) % 3) * PW + t % 3
    vv = np.arange(V)
    vz, vy, vx = vv // (win * win), (vv // win) % win, vv % win
    corner = (vz * PW + vy) * PW + vx
    hh = np.arange(2)

    def mm(a, b):
        """sum over (tap, lane half, j) of a [cb, tap, h, m, j] b [col, h, tap, j] -> [cb, m, col]"""
        return (a.transpose(0, 3, 1, 2, 4).reshape(32 * ncb, -1) @ b.transpose(0, 2, 1, 3).reshape(b.shape[0], -1).T).reshape(ncb, 32, -1)

    for bx in range(nwg):
        n0 = bx * g.cols
        p_first = n0 // V
        n = n0 + np.arange(min(g.cols, ntot - n0))
        p = n // V
        v = n - p * V
        slot = p - p_first
        if defect == "slot_short" and n0 % V:
            slot = np.maximum(slot - 1, 0)
        if f16:
            unit = (hh[None, :] * PK + slot[:, None]) * CSB + corner[v][:, None]                      # [col, h]
            idx = unit[:, :, None] + toff                                                             # [col, h, tap]
            idx_lo = idx[:, [0, 0], :] if defect == "lo_half" else idx
        else:
            unit = slot[:, None] * CK * CSB + hh[None, :] * CSB + corner[v][:, None]
            idx = unit[:, :, None, None] + (2 * CSB * np.arange(2))[None, None, :, None] + toff       # [col, h, cp, tap]
        acc = np.zeros((ncb, 32, len(n)))
        tot = np.zeros_like(acc)
        for ch in range(nch):
            # ---- the LDS image of this chunk: PK slots, zero where the slot names no peak
            if f16:
                lB = np.zeros((2, 2, PK, CSB, 8))
            else:
                lin = np.zeros((PK, CK, CSB))
            for s in range(PK):
                pp = p_first + s
                if pp >= P:
                    continue
                nbp = p_first + (s + 1) % PK
                nbp = nbp if (defect == "border_neighbour" and nbp < P and nbp != pp) else None
                c0 = CK * ch
                if f16:
                    for plane, src in ((0, gh), (1, gl)):
                        blk = _padded(src[pp, c0:c0 + 16], None if nbp is None else src[nbp, c0:c0 + 16])       # [16, PW, PW, PW]
                        lB[plane, :, s] = blk.reshape(2, 8, CSB).transpose(0, 2, 1)
                else:
                    blk = np.zeros((CK, win, win, win))
                    nb = None if nbp is None else np.zeros_like(blk)
                    for cc in range(CK):
                        if c0 + cc < cg:
                            blk[cc] = gn[pp, c0 + cc]
                            if nb is not None:
                                nb[cc] = gn[nbp, c0 + cc]
                        elif defect == "ragged_runs_on":                                              # reads on: the next peak's channels
                            src = (pp * cg + c0 + cc) * V + vv
                            blk[cc] = np.where(src < gflat.size, gflat[np.minimum(src, gflat.size - 1)], 0.0).reshape(win, win, win)
                    lin[s] = _padded(blk, nb).reshape(CK, CSB)
            # ---- this chunk's products
            if f16:
                bh, bl = lB[0].reshape(-1, 8)[idx], lB[1].reshape(-1, 8)[idx_lo]                       # [col, h, tap, j]
                ah = ah_all[:, ch].reshape(ncb, 27, 2, 32, 8)                                         # [cb, tap, h, m, j]
                al = al_all[:, ch].reshape(ncb, 27, 2, 32, 8)
                if defect != "drop_lohi":
                    acc += mm(al, bh)
                if defect != "drop_hilo":
                    acc += mm(ah, bl)
                acc += mm(ah, bh)
                flush = bool(ch & 1) or (ch + 1 == nch and defect != "flush_skipped_even_last")
                if flush or defect == "flush_every_chunk":
                    tot += acc
                if flush:
                    acc[:] = 0
            else:
                b = lin.reshape(-1)[idx]                                                              # [col, h, cp, tap]
                a = a_all[:, ch].transpose(0, 1, 2, 4, 3).reshape(ncb, 2, 28, 2, 32)[:, :, :27]       # [cb, cp, tap, h, m]
                tot += (a.transpose(0, 4, 1, 2, 3).reshape(32 * ncb, -1) @ b.transpose(0, 2, 3, 1).reshape(len(n), -1).T).reshape(acc.shape)
        # ---- epilogue: un-scale, PreHook multiply, store
        if f16:
            pu = np.full_like(p, p_first) if defect == "unscale_first_peak" else p
            val = (tot * (sp[p] * sw)).astype(F32)                                                    # the kernel's tot, in scaled units
            val = (val * (1.0 / sp[pu]).astype(F32)) * F32(1.0 / sw)
        else:
            val = tot.astype(F32)
        val = val.reshape(32 * ncb, len(n))
        o = origin[p].astype(np.int64)
        q = o + (0 if defect == "mult_no_v" else np.stack([vz[v], vy[v], vx[v]], 1))
        qin = o + np.stack([vz[v], vy[v], vx[v]], 1)
        inside = np.all((qin >= 0) & (qin < np.array([D, H, Wd])), 1)
        qc = np.clip(q, 0, np.array([D, H, Wd]) - 1)
        co = np.arange(32 * ncb)
        m = full[np.minimum(co, cx - 1)[:, None], qc[None, :, 0], qc[None, :, 1], qc[None, :, 2]].astype(F32) - F32(off)
        res = m * val
        if defect != "clamped_read":
            res = np.where(inside[None, :], res, F32(0))
        out[p[None, :], co[:cx, None], v[None, :]] = res[:cx]
        if defect == "fold_store" and cx % 32:
            out[p[None, :], (co[cx:] % cx)[:, None], v[None, :]] = res[cx:]
    return out.reshape(P, cx, win, win, win)


def emulate_case(kind, e, defect=None):
    return emulate(kind, e["gn"], e["w"], e["full"], e["off"], e["origin"], defect)
