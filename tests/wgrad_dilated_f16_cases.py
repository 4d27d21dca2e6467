"""The case list of the dilation-2 narrow-map f16x2 conv weight gradient (csrc/conv3d_wgrad_narrow_f16.hip, its dilation-2 instantiation;
m3d_conv3d_wgrad_narrow_dilated_f16x2), shared by the host and the GPU test (no GPU needed).  The contract - the fp64 reference's form, the
bound, the input families, the mutants - is tests/wgrad_f16x2_contract.py's, with n_acc = chain + folds of
m3d_conv3d_wgrad_narrow_dilated_f16x2_plan at dilation 2; only the op is new:

  dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] x[b,ci,z+2(dz-1),y+2(dy-1),x+2(dx-1)]  (zeros outside).

(batch, cin, cout, D, H, W): the smallest shapes at which each mechanism can go wrong.  The tile is tile_z x 8 x 8 (z, y, x); tile_z is
what the library's plan exports, and the cases that are built from D alone are written through it, so another tile_z still hits them.
The tiles and the slot rule do not depend on the dilation: expected_plan and supported_rule are the dilation-1 list's, with the
dilation added to the latter."""
import torch

import wgrad_narrow_f16_cases as N1
from wgrad_narrow_f16_cases import CHAIN_LIMIT, MAX_TILES, TARGET_WGS, TILE_YX, WG_THREADS, cdiv, expected_plan, tiles      # noqa: F401

F64 = torch.float64
DILATION = 2


def cases(tile_z):
    return {
        "roi7_b3":  (3, 32, 32, 7, 7, 7),              # the RoI grid: every +-2 tap has real data and padding
        "full":     (2, 32, 32, 8, 8, 8),              # full tiles
        "one_tile": (1, 32, 32, tile_z, 8, 8),         # exactly one tile, one slot; D = 2: every dz != 1 tap exactly 0
        "short":    (2, 32, 32, 3, 5, 7),              # all three extents short, H odd; D = 3: dz = 0 only z = 2 -> 0, dz = 2 only z = 0 -> 2
        "d1_co64":  (5, 32, 64, 1, 7, 7),              # D = 1; two cout blocks
        "ci96":     (1, 96, 32, 14, 14, 8),            # several y and z tiles: the halo reaches two rows and a whole z tile into its
                                                       # neighbours on both sides; three cin blocks
        "w3":       (2, 64, 96, 7, 7, 3),              # W = 3: each x-shifted tap has exactly one column pair (x = 2 -> 0, x = 0 -> 2)
        "w2":       (1, 32, 32, 4, 9, 2),              # W = 2: both x-shifted taps exactly 0; H = 9: one row in a second y tile
        "h2":       (1, 32, 32, 5, 2, 8),              # H = 2: both y-shifted taps exactly 0
        "b17":      (17, 32, 32, 7, 7, 7),             # an uneven tile count
        "slot2":    (1, 32, 32, 1100 * tile_z, 1, 1),  # 1100 tiles: two tiles per slot, 550 slots (69 partials per reduce group)
        "slot16":   (1, 32, 32, 8200 * tile_z, 1, 1),  # 8200 tiles: 16 tiles per slot, the full chain; the last slot holds 8 tiles
    }


MUTANT_CASES = list(N1.MUTANT_CASES)                   # ["one_tile", "short", "d1_co64"], as the dilation-1 list has them
FAMILY_CASE = N1.FAMILY_CASE                           # "short"
SENTINEL_CASES = list(N1.SENTINEL_CASES)               # ["roi7_b3", "ci96", "w3", "slot2"]


def zero_taps(case):
    """(axis of the 3 x 3 x 3 tap block, tap index) of every tap that is exactly 0 whatever the data: along an axis of extent n <= 2 no
    voxel has a neighbour at distance 2, so both shifted taps of that axis read the padding only"""
    _, _, _, D, H, W = case
    return [(axis, t) for axis, n in ((2, D), (3, H), (4, W)) if n <= DILATION for t in (0, 2)]


def wgrad_op_d2(gy, x):
    """dW [cout, cin, 3, 3, 3] of gy [B, cout, D, H, W] and x [B, cin, D, H, W] (fp64) of the dilation-2, padding-2 conv: tap by tap, the
    product of gy with x shifted by 2 (d - 1) along each axis"""
    gy, x = gy.to(F64), x.to(F64)
    B, cout, D, H, W = gy.shape
    cin = x.shape[1]
    dw = torch.zeros(cout, cin, 3, 3, 3, dtype=F64)
    g2 = gy.transpose(0, 1)                                              # [cout, B, D, H, W]
    x2 = x.transpose(0, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                # output voxels (z, y, x) whose input voxel (z + 2 (dz - 1), ...) lies inside the volume
                rng = []
                for n, d in ((D, dz), (H, dy), (W, dx)):
                    s = DILATION * (d - 1)
                    lo, hi = max(0, -s), min(n, n - s)
                    rng.append((lo, hi, s))
                if any(lo >= hi for lo, hi, _ in rng):
                    continue                                             # every product of this tap reads the zero padding
                (z0, z1, sz), (y0, y1, sy), (a0, a1, sx) = rng
                g = g2[:, :, z0:z1, y0:y1, a0:a1].reshape(cout, -1)
                v = x2[:, :, z0 + sz:z1 + sz, y0 + sy:y1 + sy, a0 + sx:a1 + sx].reshape(cin, -1)
                dw[:, :, dz, dy, dx] = g @ v.T
    return dw


def supported_rule(batch, cin, cout, D, H, W, dilation, tile_z):
    """the documented rule of m3d_conv3d_wgrad_narrow_dilated_f16x2_supported (include/m3d.h): dilation 1 or 2 and the dilation-1 rule"""
    return dilation in (1, 2) and N1.supported_rule(batch, cin, cout, D, H, W, tile_z)
