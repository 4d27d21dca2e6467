"""The case list of the narrow-map f16x2 conv weight gradient (csrc/conv3d_wgrad_narrow_f16.hip; m3d_conv3d_wgrad_narrow_f16x2), shared by
the host and the GPU test (no GPU needed).  The contract - the op, the fp64 reference, the bound, the input families, the mutants - is the
wide kernel's, tests/wgrad_f16x2_contract.py, with n_acc = chain + folds of m3d_conv3d_wgrad_narrow_f16x2_plan.

(batch, cin, cout, D, H, W): the smallest shapes at which each mechanism can go wrong.  The tile is tile_z x 8 x 8 (z, y, x); tile_z is
what the library's plan exports, and the cases that are built from D alone are written through it, so another tile_z still hits them."""

TILE_YX = (8, 8)
WG_THREADS = 192
TARGET_WGS = 512
MAX_TILES = 16             # tiles of a slot
CHAIN_LIMIT = 384          # consecutive MFMAs into one accumulator (the contract's hard limit is 512)


def cases(tile_z):
    return {
        "roi7_b3":  (3, 32, 32, 7, 7, 7),              # the RoI grid: 7 of 8 along y and x, an odd last z tile
        "full":     (2, 32, 32, 8, 8, 8),              # full tiles
        "one_tile": (1, 32, 32, tile_z, 8, 8),         # exactly one tile, one slot
        "short":    (2, 32, 32, 3, 5, 7),              # all three extents short; H odd: the last k-step's second row is outside
        "d1_co64":  (5, 32, 64, 1, 7, 7),              # D = 1 (every dz != 1 tap exactly 0); two cout blocks
        "ci96":     (1, 96, 32, 14, 14, 8),            # several y and z tiles; three cin blocks
        "w3":       (2, 64, 96, 7, 7, 3),              # W = 3: one quad, zero columns; 96 <- 64
        "w1":       (1, 32, 32, 4, 9, 1),              # W = 1: both x-shifted taps exactly 0
        "b17":      (17, 32, 32, 7, 7, 7),             # an uneven tile count
        "slot2":    (1, 32, 32, 1100 * tile_z, 1, 1),  # 1100 tiles: two tiles per slot, 550 slots (69 partials per reduce group)
        "slot16":   (1, 32, 32, 8200 * tile_z, 1, 1),  # 8200 tiles: 16 tiles per slot, the full chain; the last slot holds 8 tiles
    }


MUTANT_CASES = ["one_tile", "short", "d1_co64"]        # where the mutants are tried (small: the emulation runs three ops per mutant)
FAMILY_CASE = "short"                                   # the all-short case: where the GPU test runs the other input families
SENTINEL_CASES = ["roi7_b3", "ci96", "w3", "slot2"]    # three cin blocks (ci96), multi-slot (slot2, roi7_b3)


def cdiv(a, b):
    return (a + b - 1) // b


def tiles(case, tile_z):
    B, _, _, D, H, _ = case
    return B * cdiv(D, tile_z) * cdiv(H, TILE_YX[0])


def expected_plan(case, tile_z):
    """(slots, tiles_per_slot) of the documented slot rule: slots of min(16, tiles x blocks // 512) consecutive tiles"""
    _, cin, cout = case[:3]
    nt = tiles(case, tile_z)
    tps = min(MAX_TILES, max(1, nt * (cin // 32) * (cout // 32) // TARGET_WGS))
    return cdiv(nt, tps), tps


def supported_rule(batch, cin, cout, D, H, W, tile_z):
    """the documented rule of m3d_conv3d_wgrad_narrow_f16x2_supported (include/m3d.h)"""
    if min(batch, cin, cout, D, H, W) < 1 or W > TILE_YX[1] or cin % 32 or cout % 32 or cin > 4096 or cout > 4096:
        return False
    case = (batch, cin, cout, D, H, W)
    if tiles(case, tile_z) > 2 ** 30:
        return False
    return expected_plan(case, tile_z)[0] * (cin // 32) * (cout // 32) <= (2 ** 32 - 1) // WG_THREADS
