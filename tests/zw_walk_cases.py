"""The cases of the f16x2 conv's persistent unit walk (csrc/conv3d_zw.hip: a workgroup walks units l0, l0 + grid, ...; the next unit's halo
planes, weight fragments, affine table and per-window scale are handed over inside the K loop and the epilogue).  No GPU needed, and no
tests live here: tests/test_zw_walk_cases_host.py proves the table's properties against the library's own host queries,
tests/test_gpu_zw_walk.py runs it.  References and bounds are those of tests/f16x2_contract.py (zw_contract); no new bound is derived.

SMALL cases run under the tuning build's grid override (option tune_zw_grid = G: min(G, units) workgroups), at every G of `grids`:
  G = 1           one workgroup walks every unit: both parities of the affine table reused, every cout-group, tile and batch transition
  G = 2           (ncg = 2) the cout group is constant along a walk;  G = 3, 5: it alternates
  G = 8, 9        rem = 0 / rem = 1 in zw_xcd_contiguous
  G = units - 1   one workgroup has two units, the others one: the uneven tail
  G = units       today's one-unit launch, the anchor
RELEASE cases run on the stock library with no override: more than 512 units, so that 256 CUs walk at least 3 units per workgroup.

Shapes are (B, cin, cout, D, H, W) of the conv the kernel runs, except `dgrad`: there they are the FORWARD layer's and the kernel runs the
backward-data conv cout -> cin.  (The forward layer 32 -> 64 would give the walk one cout group and 16 units; 70 -> 64 gives the
backward-data conv 4 chunks, a 6-channel second group and 32 units.)

Integer operands (x in 0..7, or -7..7 where signed; w in -3..3; power-of-two scales, integer shifts): every V_k = d_a -+ d_b is an integer
of magnitude <= 14, every U_k a half-integer of magnitude <= 4.5, both exact in one fp16 piece; an accumulator holds at most
9 cin 14 9 half-units (in units of the two operand scales), the Winograd-z combination three times that: below 2^24, so every product
and every partial sum is exact in fp32 whatever the order, and the result must EQUAL the fp64 reference."""
import collections

import torch
import torch.nn.functional as F

import conv_train_cases as CT
import f16x2_contract as K

F64 = torch.float64
CAP_FLOP = 2.5e9                 # small cases, per reference conv (tests/direct_conv_cases.py's cap)
CAP_FLOP_RELEASE = 2 * 2.0e9     # release cases: about 2 GMAC
CUS = 256                        # the MI355X

# form: "conv" (<XB, false>), "pool" (<32, true>), "dgrad" (<32, false> on ZwConv3d.dgrad_of), "strip" (<32, false> + col_bound),
# "strip_prepare" (<32, false, true>)
Case = collections.namedtuple("Case", "name form shape units signed why")

STRIP = dict(cin=32, cout=32, n=10, P=5)          # five 10^3 windows: ops.strip_geometry(10, 2, 5) = (pitch 12, lead 1, L 64)
STRIP_MAP = (12, 14, 16)                           # the map (MD, MH, MW) the prepared strip of `strip_prepare` is cut from
# window origins in that map (z, y, x): inside, sticking out below 0 on every axis, out above the map on every axis, out on z only, on x only
STRIP_ORIGINS = ((1, 2, 3), (-4, -3, -5), (7, 9, 11), (-9, 0, 2), (2, 4, -8))

SMALL = collections.OrderedDict((c.name, c) for c in (
    Case("xb32", "conv", (2, 48, 70, 3, 5, 37), 32, True,
         "3 chunks (odd: the last chunk on buffer 0), ncg = 2 with a 6-channel second group, ragged on z, y and x, 2 batch items"),
    Case("xb32_narrow", "conv", (2, 16, 66, 4, 8, 61), 32, True,
         "one chunk at the 32-wide tile, full y and z tiles, W % 4 != 0, a 2-channel second group: in every other unit seven of the eight "
         "waves have no epilogue work and run ahead into the next unit's staging and affine table"),
    Case("xb16", "conv", (2, 16, 96, 3, 9, 20), 32, True,
         "one chunk (`last` at c = 0: all four next-unit planes requested at taps 0-2), the 16 x 2 column blocks"),
    Case("xb16_w21", "conv", (2, 16, 96, 3, 9, 21), 32, True, "xb16 with W % 4 != 0: the scalar-store path"),
    Case("pool", "pool", (2, 32, 70, 4, 8, 48), 32, False, "fused pool, a ragged second x tile, ncg = 2"),
    Case("dgrad", "dgrad", (2, 70, 64, 3, 5, 37), 32, True, "the dgrad pack under a walk (backward-data 64 -> 70: 4 chunks, ncg = 2)"),
    Case("strip", "strip", (1, 32, 32, 10, 10, 64), 30, True,
         "one scale per window, each window x its own power of two: consecutive units carry different xs / inv_e"),
    Case("strip_prepare", "strip_prepare", (1, 32, 32, 10, 10, 64), 30, True, "the PREP epilogue; windows sticking out of the map"),
))

RELEASE = collections.OrderedDict((c.name, c) for c in (
    Case("release", "conv", (2, 16, 70, 13, 17, 97), 560, True,
         "560 units: 187 workgroups on 256 CUs, 186 walk 3 units and one walks 2 (the ragged last round); W % 4 != 0"),
    Case("release_pool", "pool", (2, 16, 130, 10, 22, 66), 540, False, "540 units, ncg = 3 with a 2-channel third group: 180 workgroups x 3"),
))
CASES = collections.OrderedDict(list(SMALL.items()) + list(RELEASE.items()))

WALK_FAMILIES = ("benign", "heavy")                # (b) walk-independence
BOUND_FAMILIES = ("benign", "outlier24", "quiet")  # (c) bounded under a walk
BOUND_GRIDS = (1, 3)


def grids(case):
    """the grid sizes a small case runs at"""
    return sorted({1, 2, 3, 5, 8, 9, case.units - 1, case.units})


def kernel_dims(case):
    """(B, cin, cout, D, H, W) of the conv the KERNEL runs"""
    B, cin, cout, D, H, W = case.shape
    return (B, cout, cin, D, H, W) if case.form == "dgrad" else case.shape


def flop(case):
    B, cin, cout, D, H, W = case.shape
    return 2.0 * 27 * B * cin * cout * D * H * W


def exact_half_units(case):
    """the proof obligation of the integer cases (module docstring): the largest accumulator magnitude in half-units"""
    return 9 * kernel_dims(case)[1] * 14 * 9


# ------------------------------------------------------------------ the walk, restated
def xcd_contiguous(bid, n):
    """zw_xcd_contiguous of conv3d_zw.hip: workgroup id -> the first unit of its walk"""
    per, rem = n >> 3, n & 7
    xcd, idx = bid & 7, bid >> 3
    return xcd * per + min(xcd, rem) + idx


def walk(units, grid):
    """the units every workgroup of a `grid`-workgroup launch visits, in order: [[l0, l0 + grid, ...] per workgroup]"""
    return [list(range(xcd_contiguous(b, grid), units, grid)) for b in range(grid)]


def stock_grid(units, cus=CUS):
    """launch_zw's own workgroup count: every workgroup the same number of units where the count allows it"""
    rounds = (units + cus - 1) // cus
    return (units + rounds - 1) // rounds


# ------------------------------------------------------------------ operands
def _gen(case, salt=0):
    return torch.Generator().manual_seed(100 * list(CASES).index(case.name) + salt)


def epilogue_operands(cout, gen):
    """power-of-two scale, integer shift (test_gpu_direct_conv.epilogue_operands): every step of the epilogue is exact"""
    scale = 2.0 ** torch.randint(-1, 3, (cout,), generator=gen).to(torch.float32)
    shift = torch.randint(-8, 9, (cout,), generator=gen).to(torch.float32)
    return scale, shift


def strip_of(wins, pitch, lead, L):
    """[P, cin, n, n, n] windows -> the strip [cin, n, n, L], zero between the windows"""
    cin, n = wins.shape[1], wins.shape[2]
    s = torch.zeros(cin, n, n, L)
    for p in range(wins.shape[0]):
        s[..., lead + p * pitch:lead + p * pitch + n] = wins[p]
    return s


def window_powers(P):
    """each window's own power of two, 2^-6 .. 2^6"""
    return 2.0 ** torch.linspace(-6, 6, P).round()


def operand_shapes(case):
    """(operand shape, FORWARD-layout weight shape): x [B, cin, ...] (conv, pool), gy [B, cout, ...] (dgrad), windows [P, cin, n, n, n]"""
    B, cin, cout, D, H, W = case.shape
    if case.form in ("strip", "strip_prepare"):
        return (STRIP["P"], STRIP["cin"]) + (STRIP["n"],) * 3, (STRIP["cout"], STRIP["cin"], 3, 3, 3)
    return (B, cout if case.form == "dgrad" else cin, D, H, W), (cout, cin, 3, 3, 3)


def integer_operands(case):
    """dict(a, w, scale, shift) as in conv_train_cases.integer_inputs: a in 0..7 (-7..7 signed), w in -3..3; strips: each window x its power
    of two.  scale / shift belong to the kernel's output channels"""
    g = _gen(case)
    ashape, wshape = operand_shapes(case)
    a = torch.randint(-7 if case.signed else 0, 8, ashape, generator=g).float()
    w = torch.randint(-3, 4, wshape, generator=g).float()
    if case.form in ("strip", "strip_prepare"):
        a = a * window_powers(ashape[0]).view(-1, 1, 1, 1, 1)
    scale, shift = epilogue_operands(kernel_dims(case)[2], g)
    return dict(a=a, w=w, scale=scale, shift=shift)


def random_operands(case, family):
    """dict(a, w, scale, shift) of a family of f16x2_contract.inputs; strips: a quiet half inside every window, magnitudes 2^-20 .. 2^20
    (tests/test_gpu_f16x2_range.py::test_zw_strip_meets_the_contract_per_window)"""
    ashape, wshape = operand_shapes(case)
    a, w = K.inputs(family, ashape, wshape, 7 + list(CASES).index(case.name), signed=case.signed)
    if case.form in ("strip", "strip_prepare"):
        n, P = ashape[2], ashape[0]
        a[..., :n // 2] *= 2.0 ** -30
        a *= (2.0 ** torch.linspace(-20, 20, P)).view(P, 1, 1, 1, 1)
    g = _gen(case, 1)
    cout = kernel_dims(case)[2]
    return dict(a=a, w=w, scale=torch.rand(cout, generator=g) + 0.5, shift=torch.randn(cout, generator=g))


def prepare_operands(case):
    """the layer below of `strip_prepare`: xnext / norm [cout, MD, MH, MW] with exact zeros, BatchNorm scales of both signs, the PreHook
    offset, the windows' origins (tests/test_gpu_prm.py::test_quad_prepare_kernel_writes_the_element_kernels_strip_bit_for_bit)"""
    g = _gen(case, 2)
    shape = (STRIP["cout"],) + STRIP_MAP
    xnext = torch.randn(shape, generator=g) * (torch.rand(shape, generator=g) > 0.3)
    norm = torch.rand(shape, generator=g) * (torch.rand(shape, generator=g) > 0.2)
    scale = torch.rand((STRIP["cout"],), generator=g) - 0.4
    return dict(xnext=xnext, norm=norm, scale=scale, up_off=torch.tensor([0.125]), origin=torch.tensor(STRIP_ORIGINS, dtype=torch.int32))


def kernel_weight(case, w):
    """the weight of the conv the kernel runs, as a forward conv [cout_k, cin_k, 3, 3, 3]"""
    return CT.dgrad_weight(w) if case.form == "dgrad" else w


# ------------------------------------------------------------------ references (fp64)
def conv64(case, a, w):
    """the plain conv of the form: conv3d, or the transposed conv of the forward layer's weight (what autograd's backward-data is); strips:
    every window on its own [P, cout, n, n, n]"""
    if case.form == "dgrad":
        return K.dgrad_op(a.to(F64), w.to(F64))
    return K.conv3d_op(a.to(F64), w.to(F64))


def epilogue64(y, scale, shift, pool=False):
    v = torch.relu(y * scale.to(F64).view(1, -1, 1, 1, 1) + shift.to(F64).view(1, -1, 1, 1, 1))
    return F.max_pool3d(v, 2, 2) if pool else v


_cache = {}


def integer_reference(name):
    """(operands, plain fp64 result, fp64 result with scale, shift, ReLU [and the pool]); computed once, shared, never modified"""
    key = ("int", name)
    if key not in _cache:
        c = CASES[name]
        o = integer_operands(c)
        y = conv64(c, o["a"], o["w"])
        _cache[key] = (o, y, epilogue64(y, o["scale"], o["shift"], pool=(c.form == "pool")))
    return _cache[key]


def contract(name, family):
    """(operands, list of (y, E, C)) of zw_contract with the swept bound max |a|: the pooled form with scale, shift and ReLU, the un-pooled
    and dgrad forms with scale and shift, the strips one entry per window with the window's own bound"""
    key = ("rnd", name, family)
    if key not in _cache:
        c = CASES[name]
        o = random_operands(c, family)
        a, wk = o["a"], kernel_weight(c, o["w"])
        if c.form in ("strip", "strip_prepare"):
            res = [K.zw_contract(a[p:p + 1], wk, float(a[p].abs().max())) for p in range(a.shape[0])]
        elif c.form == "pool":
            res = [K.zw_contract(a, wk, float(a.abs().max()), scale=o["scale"], shift=o["shift"], relu=True, pool=True)]
        else:
            res = [K.zw_contract(a, wk, float(a.abs().max()), scale=o["scale"], shift=o["shift"])]
        _cache[key] = (o, res)
    return _cache[key]


def unit_of(case, index):
    """the walk unit that writes output element (b, co, z, y, x) of the kernel's un-pooled output (pooled: pass 2 x the pooled z, y, x):
    units are (cout group fastest, x tile, y tile, z tile, batch item)"""
    B, cin, cout, D, H, W = kernel_dims(case)
    xb = 32 if W >= 24 else 16
    ty = 4 * (32 // xb)
    b, co, z, y, x = (int(v) for v in index)
    ncg, tx_n, ty_n, tz_n = (cout + 63) // 64, (W + xb - 1) // xb, (H + ty - 1) // ty, (D + 1) // 2
    return co // 64 + ncg * (x // xb + tx_n * (y // ty + ty_n * (z // 2 + tz_n * b)))
