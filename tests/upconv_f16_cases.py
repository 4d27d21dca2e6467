"""The cases of the up-conv's f16x2 forward and of the fused mask-head tail (csrc/upconv3d_f16.hip, ops.UpConvF16), with fp64 references and
the per-element bounds of tests/f16x2_contract.py.  No GPU needed.

  plain   y[r,co,2z+a,2y+b,2x+c] = bu[co] + sum_ci x[r,ci,z,y,x] W[ci,co,a,b,c]  [ReLU]       a = x (bound A = in_max), b = W (B = fl(max|W|))
  fused   l[r,k,...] = bc[k] + sum_co wc[k,co] max(y[r,co,...], 0);  out = sigmoid(l) or l

Up-conv element:  E_u = c1 2^-22 C + F + C3 n_acc 2^-24 (C + F) + 2^-24 |y64|   (f16x2_contract.bound), with the kernel's constants, from
its code (not from a fit):
  c1 = 3 + 2^-22 (written 3.01): x and W themselves are cut - neither operand is rounded to fp32 before the cut;
  n_acc = 3 Cin / 16: one accumulator takes the three MFMAs of each of the Cin / 16 k steps (with more than 256 input channels the tile
      is re-staged, the accumulator goes on); after them the kernel does ONE fp32 operation, fma(acc, 1 / (s_a s_b), bias): the power of
      two is exact, the one rounding is the add's - the LAST operation, the bound's 2^-24 |y| term.  So nothing is added to 3 Cin / 16.
ReLU is 1-Lipschitz.  Where C == 0 the element is exactly the bias (or 0).

Fused logit:  E_l[k] = sum_co |wc[k,co]| E_u[co] + gamma_m (sum_co |wc[k,co]| (u64[co] + E_u[co]) + |bc[k]|),  u64 = max(y64, 0),
gamma_m = m 2^-24 / (1 - m 2^-24) with
  m = Cout + 2: the Cout terms of the classifier sum (fp32 FMA, any order: Cout), + 1 for the bias add, + 1 for the ONE partial sum the
      kernel's fixed order adds: every lane half sums its channels (rows 4h + {0..3} + 8i of each 32-channel block, blocks ascending), then
      the two halves are added.
The sigmoid has no bound of its own: sigmoid = 1 must equal torch.sigmoid of the same call's sigmoid = 0 output bit for bit."""
import torch

from f16x2_contract import cut, emulate, terms, inputs, C2, C3            # noqa: F401  (cut: re-exported for the tests)

F64 = torch.float64
C1 = 3.01


def n_acc(cin):
    return 3 * cin / 16


def m_fused(cout):
    return cout + 2


def gamma(m):
    return m * 2.0 ** -24 / (1.0 - m * 2.0 ** -24)


CUS = 256                                     # compute units of the chip: the walk case is stated against it
COLS = 64                                     # columns (voxels of the RoI batch, R D H W in all) of one workgroup
# (R, Cin, Cout, D, H, W, K)
CASES = {
    "one": (1, 16, 1, 1, 1, 1, 1),            # one voxel, one channel, class-agnostic
    "ragged": (3, 48, 40, 2, 3, 5, 3),        # three 16-chunks (an odd k-step count), Cout off every tile edge, odd extents
    "roi_grid": (2, 64, 64, 7, 7, 7, 2),      # V = 343: no row is a 16-byte multiple; a 64-column tile spans the two RoIs
    "wide_row": (2, 32, 72, 3, 4, 33, 2),     # a row longer than a tile
    "shipped": (1, 256, 256, 7, 7, 7, 2),     # the real channel counts, one RoI
    # two workgroups of 64 KB LDS per CU: 2 CUS = 512 workgroup slots.  97 RoIs x 343 voxels = 33271 columns = 519 full workgroups + one
    # of 55 columns: 520 = 512 + 8, a second, partial round whose last workgroup is ragged
    "walk": (97, 16, 8, 7, 7, 7, 2),
}
# beside the issue's six: more input channels than one staged chunk of 256 (the tile is re-staged inside every channel block), 17 k steps
EXTRA_CASES = {"chunks": (2, 272, 5, 2, 3, 3, 2)}
assert (CASES["walk"][0] * 343 + COLS - 1) // COLS == 2 * CUS + 8 and CASES["walk"][0] * 343 % COLS == 55
FAMILIES = ("benign", "heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below")
CUT_MUTANTS = ("hi_only", "drop_hilo", "lo_unscaled")
# a (case, family) on which each cut mutant must break E_u (tests/test_upconv_f16_host.py)
MUTANT_SITES = {"hi_only": ("roi_grid", "benign"), "drop_hilo": ("shipped", "heavy"), "lo_unscaled": ("ragged", "quiet")}
GEOMETRY_DEFECTS = ("parity_swap", "no_relu", "class_swap")


def up_op(x, w):
    """ConvTranspose3d(kernel 2, stride 2, padding 0), bilinear in (x, w), fp64"""
    return torch.nn.functional.conv_transpose3d(x.to(F64), w.to(F64), stride=2)


def make(case, family, seed=5):
    """(x, w, bu, wc, bc): x >= 0 (the trunk's output is ReLU'd), the up-conv weight and bias, the classifier [K, Cout] and its bias"""
    R, cin, cout, D, H, W, K = CASES.get(case) or EXTRA_CASES[case]
    x, w = inputs(family, (R, cin, D, H, W), (cin, cout, 2, 2, 2), seed, signed=False)
    g = torch.Generator().manual_seed(seed + 1)
    return x, w, torch.randn(cout, generator=g), torch.randn(K, cout, generator=g) * 0.2, torch.randn(K, generator=g)


def integer_inputs(case, seed=3):
    """x, W, wc in [-3, 3], integer biases: the cut of a small integer is exact, every up-conv partial sum stays below 256 9 + 5 and every
    logit below 256 3 2309 < 2^24, so the fp32 accumulation, the exact un-scaling and both bias adds are exact: bit-equal to fp64"""
    R, cin, cout, D, H, W, K = CASES.get(case) or EXTRA_CASES[case]
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, s: torch.randint(lo, hi + 1, s, generator=g).float()
    return ri(-3, 3, (R, cin, D, H, W)), ri(-3, 3, (cin, cout, 2, 2, 2)), ri(-5, 5, (cout,)), ri(-3, 3, (K, cout)), ri(-5, 5, (K,))


def _chan(v):
    return v.to(F64).view(1, -1, 1, 1, 1)


def finish(acc, bu=None, relu=False):
    """the plain epilogue on an fp64 sum"""
    if bu is not None:
        acc = acc + _chan(bu)
    return torch.relu(acc) if relu else acc


def classify(u, wc, bc=None):
    """the classifier on u [R, Cout, ...] (fp64): [R, K, ...]"""
    l = torch.einsum("kc,rcdhw->rkdhw", wc.to(F64), u.to(F64))
    return l if bc is None else l + _chan(bc)


def bounds(x, w, in_bound=None):
    """(A, B) of the kernel: the input bound the caller gives (default: max|x|, what a sweep gives) and fl(max|W|)"""
    return (float(x.abs().max()) if in_bound is None else float(in_bound)), float(w.abs().max())


def bound_E(cin, C, Sa, Sb, n, A, B, y):
    """E_u of every output: the formula of f16x2_contract.bound with this kernel's (c1, n_acc)"""
    A, B = torch.as_tensor(A, dtype=F64), torch.as_tensor(B, dtype=F64)
    Fq = C2 * 2.0 ** -39 * (A * Sb + B * Sa) + 2.0 ** -77 * n * A * B
    return C1 * 2.0 ** -22 * C + Fq + C3 * n_acc(cin) * 2.0 ** -24 * (C + Fq) + 2.0 ** -24 * y.abs()


def contract_up(x, w, bu=None, relu=False, in_bound=None):
    """(fp64 reference, E_u, C) of the plain epilogue with operand bound in_bound (None: max|x|)"""
    A, B = bounds(x, w, in_bound)
    C, Sa, Sb, n = terms(up_op, x, w)
    y = finish(up_op(x, w), bu, relu)
    return y, bound_E(x.shape[1], C, Sa, Sb, n, A, B, y), C            # (ReLU is 1-Lipschitz)


def contract_fused(x, w, bu, wc, bc, in_bound=None):
    """(fp64 logits, E_l) of the fused epilogue"""
    u, Eu, _ = contract_up(x, w, bu, True, in_bound)
    wa = wc.to(F64).abs()
    l = classify(u, wc, bc)
    El = classify(Eu, wa) + gamma(m_fused(w.shape[1])) * (classify(u + Eu, wa) + _chan(bc).abs())
    return l, El


def emulated(x, w, bu=None, relu=False, in_bound=None, mutant=None):
    """the plain epilogue with exact accumulation (fp64): the three products of the cut operands, then bias and ReLU"""
    A, B = bounds(x, w, in_bound)
    return finish(emulate(up_op, x, w, A, B, mutant), bu, relu)


def defective_logits(x, w, bu, wc, bc, defect):
    """the fused logits in fp64 with a seeded geometry defect: the parities b and c swapped (out[.., 2y+b, 2x+c] <-> [.., 2y+c, 2x+b]),
    the ReLU left out, the class rows of the classifier swapped (the last two)"""
    y = finish(up_op(x, w), bu, relu=defect != "no_relu")
    if defect == "class_swap":
        K = wc.shape[0]
        perm = list(range(K))
        perm[-1], perm[-2] = perm[-2], perm[-1]
        return classify(y, wc[perm], bc[perm])
    l = classify(y, wc, bc)
    if defect == "parity_swap":
        R, K, D2, H2, W2 = l.shape
        t = l.reshape(R, K, D2, H2 // 2, 2, W2 // 2, 2).transpose(4, 6)
        return t.reshape(R, K, D2, H2, W2)
    return l


_cache = {}


def reference(case, family):
    """(x, w, bu, wc, bc, y64 (ReLU'd), E_u, C, l64, E_l), computed once and shared (never modified)"""
    key = (case, family)
    if key not in _cache:
        x, w, bu, wc, bc = make(case, family)
        y, Eu, C = contract_up(x, w, bu, True)
        wa = wc.to(F64).abs()
        l = classify(y, wc, bc)
        El = classify(Eu, wa) + gamma(m_fused(w.shape[1])) * (classify(y + Eu, wa) + _chan(bc).abs())
        _cache[key] = (x, w, bu, wc, bc, y, Eu, C, l, El)
    return _cache[key]


def worst(got, ref, E):
    """largest |got - ref| / E; an element whose bound is 0 must be exact (inf if it is not)"""
    err = (got.to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / torch.where(E > 0, E, torch.ones_like(E)))
    r = torch.where((E == 0) & (err > 0), torch.full_like(err, float("inf")), r)
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0
