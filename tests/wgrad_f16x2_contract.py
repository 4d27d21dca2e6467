"""The per-element accuracy contract of the f16x2 conv weight gradient (csrc/conv3d_wgrad_f16.hip; m3d_conv3d_wgrad_f16x2), in the form of
tests/f16x2_contract.py, with the fp64 reference and the case list of the host and GPU tests (no GPU needed).

The op, bilinear in (a = gy, b = x):  dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] x[b,ci,z+dz-1,y+dy-1,x+dx-1]  (zeros outside).

The constants, derived from the kernel's code:
  * c1 = 3 + 2^-22 (3.01, as the fc row of f16x2_contract rounds it): both operands are raw fp32 tensors that the staging code multiplies
    by the power of two of their bound (exact) and cuts - the kernel rounds neither operand before the cut, so no 0.25 is added.
    A = max |gy|, B = max |x|: ONE scale per operand tensor (the largest slot of d_gy_max / d_in_max).
  * n_acc = chain + folds of m3d_conv3d_wgrad_f16x2_plan for the shape: `chain` = tiles_per_slot x 8 rows x 3 products, the MFMAs one
    accumulator takes in its split-K slot (each truncates: c3 = 2 per step); `folds` = ceil(slots / 8) + 7 fp32 round-to-nearest adds of
    the reduce launch on the longest path of an output (half a truncation step each, counted as whole ones) + the 2 scale multiplies
    (exact, counted).
  * 2^-24 |y|: the rounding of the last operation (contained in the above when the last multiply is exact; kept, as everywhere).
Where C == 0 (no product of the output is non-zero) every term is exactly 0 and so is the output."""
import torch

from f16x2_contract import cut, emulate, terms, inputs, C2, C3      # noqa: F401  (cut and emulate: re-exported for the tests)

F64 = torch.float64
C1 = 3.01
CHAIN_MAX = 512            # the issue's limit on consecutive MFMAs into one accumulator
TILE = (2, 4, 16)          # the kernel's voxel tile (z, y, x): the coverage rule below is written against it; the host test checks
ROWS_PRODUCTS = 8 * 3      # every case against m3d_conv3d_wgrad_f16x2_plan, so a moved tile fails there

FAMILIES = ["benign", "heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below", "zero"]
MUTANTS = ["hi_only", "drop_hilo", "scale_up", "lo_unscaled"]

# (batch, cin, cout, D, H, W): the smallest shapes at which each mechanism can go wrong
CASES = {
    "ragged3":   (1, 32, 32, 5, 9, 35),       # >= 2 tiles on each axis, the last ragged on each axis; W % 8 = 3; 27 slots: split reduction
    "one_tile":  (1, 32, 32, 2, 4, 16),       # a single tile: a single slot
    "d1_w1":     (1, 32, 32, 1, 6, 17),       # D = 1; W % 8 = 1
    "hsmall_w2": (1, 32, 32, 3, 2, 18),       # H smaller than a tile; W % 8 = 2
    "w4":        (1, 32, 32, 2, 4, 20),
    "w5":        (1, 32, 32, 2, 5, 21),
    "b2_w6":     (2, 32, 32, 3, 4, 22),       # batch 2
    "b3_w7":     (3, 32, 32, 2, 3, 23),       # batch 3
    "co64":      (1, 32, 64, 3, 5, 19),       # 64 <- 32: two cout blocks
    "ci96":      (1, 96, 32, 2, 6, 9),        # 32 <- 96: three cin blocks
    "co96_ci64": (1, 64, 96, 2, 5, 9),        # 96 <- 64
    "slot2":     (1, 32, 32, 1100, 1, 17),    # 1100 tiles: two tiles per slot, 550 slots (69 partials per reduce group)
    "slot16":    (1, 32, 32, 16400, 1, 1),    # 8200 tiles: 16 tiles per slot, the full chain; the last slot holds 8 tiles
    "roi7_b5":   (5, 32, 32, 7, 7, 7),        # the 7^3 RoI maps of the mask head, batch 5
}
MUTANT_CASES = ["one_tile", "d1_w1", "co64"]  # where the mutants are tried (small: the emulation runs three ops per mutant)


def flops(case):
    B, cin, cout, D, H, W = case
    return 2 * 27 * cin * cout * B * D * H * W


def wgrad_op(gy, x):
    """dW [cout, cin, 3, 3, 3] of gy [B, cout, D, H, W] and x [B, cin, D, H, W] (fp64): tap by tap, the product of gy with the shifted x"""
    gy, x = gy.to(F64), x.to(F64)
    B, cout, D, H, W = gy.shape
    cin = x.shape[1]
    dw = torch.zeros(cout, cin, 3, 3, 3, dtype=F64)
    g2 = gy.transpose(0, 1)                                              # [cout, B, D, H, W]
    x2 = x.transpose(0, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                # output voxels (z, y, x) whose input voxel (z + dz - 1, ...) lies inside the volume
                rng = []
                for n, d in ((D, dz), (H, dy), (W, dx)):
                    lo, hi = max(0, 1 - d), min(n, n + 1 - d)
                    rng.append((lo, hi, d - 1))
                if any(lo >= hi for lo, hi, _ in rng):
                    continue                                             # every product of this tap reads the zero padding
                (z0, z1, sz), (y0, y1, sy), (a0, a1, sx) = rng
                g = g2[:, :, z0:z1, y0:y1, a0:a1].reshape(cout, -1)
                v = x2[:, :, z0 + sz:z1 + sz, y0 + sy:y1 + sy, a0 + sx:a1 + sx].reshape(cin, -1)
                dw[:, :, dz, dy, dx] = g @ v.T
    return dw


def bound(n_acc, C, Sa, Sb, n, A, B, y):
    """E of every output, the formula of f16x2_contract.bound with this kernel's c1 and n_acc (gain 1)"""
    A, B = torch.as_tensor(A, dtype=F64), torch.as_tensor(B, dtype=F64)
    F = C2 * 2.0 ** -39 * (A * Sb + B * Sa) + 2.0 ** -77 * n * A * B
    return C1 * 2.0 ** -22 * C + F + C3 * n_acc * 2.0 ** -24 * (C + F) + 2.0 ** -24 * y.abs()


def make_inputs(name, case, seed, relu_x):
    """(gy, x) fp32: x of the input family (signed, or ReLU'd like an activation), gy signed; `zero`: x = 0"""
    B, cin, cout, D, H, W = case
    x, gy = inputs(name, (B, cin, D, H, W), (B, cout, D, H, W), seed, signed=not relu_x)
    return gy.contiguous(), x.contiguous()


def contract(gy, x, n_acc):
    """(fp64 reference, E, C, A, B)"""
    A, B = float(gy.abs().max()), float(x.abs().max())
    y = wgrad_op(gy, x)
    C, Sa, Sb, n = terms(wgrad_op, gy, x)
    return y, bound(n_acc, C, Sa, Sb, n, A, B, y), C, A, B


def integer_inputs(case, seed):
    """integers in [-8, 8]: the cut is exact (lo = 0), every product and sum is an integer below 2^24 times the scales: truncation cannot act"""
    B, cin, cout, D, H, W = case
    assert 64 * B * D * H * W < 2 ** 24
    g = torch.Generator().manual_seed(seed)
    gy = torch.randint(-8, 9, (B, cout, D, H, W), generator=g).float()
    x = torch.randint(-8, 9, (B, cin, D, H, W), generator=g).float()
    return gy, x


def expected_plan(case):
    """(slots, tiles_per_slot) the coverage rule assumes for a case: tiles of TILE, slots of min(16, tiles x blocks // 512) tiles"""
    B, cin, cout, D, H, W = case
    cdiv = lambda a, b: (a + b - 1) // b
    nt = B * cdiv(D, TILE[0]) * cdiv(H, TILE[1]) * cdiv(W, TILE[2])
    tps = min(16, max(1, nt * (cin // 32) * (cout // 32) // 512))
    return cdiv(nt, tps), tps


def supported_rule(batch, cin, cout, D, H, W):
    """the documented rule of m3d_conv3d_wgrad_f16x2_supported (include/m3d.h)"""
    if min(batch, cin, cout, D, H, W) < 1 or cin % 32 or cout % 32 or cin > 4096 or cout > 4096:
        return False
    cdiv = lambda a, b: (a + b - 1) // b
    nt = batch * cdiv(D, 2) * cdiv(H, 4) * cdiv(W, 16)
    if nt > 2 ** 30:
        return False
    return expected_plan((batch, cin, cout, D, H, W))[0] * (cin // 32) * (cout // 32) <= (2 ** 32 - 1) // 192      # workgroups of 192 threads
