"""CPU: the case table of tests/zw_walk_cases.py has the properties the GPU walk tests rely on - asked of the library's own host queries
(m3d_conv3d_zw_launch_units, m3d_conv3d_zw_supported, m3d_prm_strip_geometry), so that a moved tile size or width rule fails here and not
silently on the GPU - and a restatement of the walk (zw_xcd_contiguous + the stride) visits every unit exactly once at every grid the
table uses, so that a failure on the GPU points at the kernel and not at the table."""
import ctypes as C
import math

import pytest

import zw_walk_cases as T

M3D_EUNSUPPORTED = -4


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import LIB_PATH
    lib = C.CDLL(LIB_PATH)
    lib.m3d_conv3d_zw_launch_units.restype = C.c_longlong
    lib.m3d_prm_strip_geometry.restype = C.c_int64
    return lib


def cdiv(a, b):
    return (a + b - 1) // b


def tiles(c):
    """(x, y, z) tiles of the kernel's launch and its tile, by the kernel's width rule (checked against the library in test_unit_counts)"""
    B, cin, cout, D, H, W = T.kernel_dims(c)
    xb = 32 if W >= 24 else 16
    ty = 4 * (32 // xb)
    return (cdiv(W, xb), cdiv(H, ty), cdiv(D, 2)), (xb, ty, 2)


def ncg(c):
    return cdiv(T.kernel_dims(c)[2], 64)


def test_unit_counts(L):
    for c in T.CASES.values():
        B, cin, cout, D, H, W = T.kernel_dims(c)
        assert L.m3d_conv3d_zw_supported(cin, cout, D, H, W, int(c.form == "pool")) == 1, c.name
        units = L.m3d_conv3d_zw_launch_units(B, cin, cout, D, H, W)
        assert units == c.units, (c.name, units)
        (tx, ty, tz), _ = tiles(c)
        assert units == B * ncg(c) * tx * ty * tz, c.name                 # the restated tile rule is the library's
    for c in T.SMALL.values():
        assert 24 <= c.units <= 64, c.name
    assert len({c.name for c in T.CASES.values()}) == len(T.CASES) == len(T.SMALL) + len(T.RELEASE)


def test_strip_geometry_is_the_tables(L):
    pitch, lead = C.c_int32(0), C.c_int32(0)
    n, P = T.STRIP["n"], T.STRIP["P"]
    Ls = L.m3d_prm_strip_geometry(n, 2, P, C.byref(pitch), C.byref(lead))
    for name in ("strip", "strip_prepare"):
        B, cin, cout, D, H, W = T.SMALL[name].shape
        assert (B, cin, cout, D, H, W) == (1, T.STRIP["cin"], T.STRIP["cout"], n, n, int(Ls))
    assert pitch.value % 4 == 0 and pitch.value >= n + lead.value + 1 and lead.value >= 1      # a zero column on both sides of every window
    assert len(T.STRIP_ORIGINS) == P
    # windows 0 .. P - 1 lie in different x tiles of the 32-wide kernel: a walk along x changes the window scale
    assert len({(lead.value + p * pitch.value) // 32 for p in range(P)}) >= 2
    # the windows' powers of two differ between neighbours
    pw = T.window_powers(P).tolist()
    assert min(pw) == 2.0 ** -6 and max(pw) == 2.0 ** 6 and all(a != b for a, b in zip(pw, pw[1:]))
    # at least one window sticks out of the map, on every side of every axis between them, and one lies inside
    MD = T.STRIP_MAP
    out_lo = [any(o[k] - 1 < 0 for o in T.STRIP_ORIGINS) for k in range(3)]
    out_hi = [any(o[k] + n + 1 > MD[k] for o in T.STRIP_ORIGINS) for k in range(3)]
    assert all(out_lo) and all(out_hi)
    assert any(all(o[k] - 1 >= 0 and o[k] + n + 1 <= MD[k] for k in range(3)) for o in T.STRIP_ORIGINS)
    assert MD[2] >= 4


def test_tiles_batch_and_cout_groups():
    for c in T.SMALL.values():
        t, _ = tiles(c)
        if c.form in ("strip", "strip_prepare"):
            assert T.kernel_dims(c)[0] == 1 and ncg(c) == 1
            continue
        assert min(t) >= 2, (c.name, t)
        assert T.kernel_dims(c)[0] == 2 and ncg(c) >= 2, c.name
    for c in T.RELEASE.values():
        assert T.kernel_dims(c)[0] == 2 and ncg(c) >= 2 and T.kernel_dims(c)[1] == 16
    # a partial last cout group, and ragged tiles on every axis, in at least one un-pooled and the dgrad case
    for name in ("xb32", "dgrad"):
        c = T.SMALL[name]
        B, cin, cout, D, H, W = T.kernel_dims(c)
        _, (bx, by, bz) = tiles(c)
        assert cout % 64 != 0 and W % bx != 0 and H % by != 0 and D % bz != 0, name


def test_chunks_and_widths():
    chunks = {T.kernel_dims(c)[1] // 16 for c in T.SMALL.values()}
    assert 1 in chunks and 2 in chunks and any(k >= 3 and k % 2 == 1 for k in chunks), chunks
    assert all(T.kernel_dims(c)[1] % 16 == 0 for c in T.CASES.values())
    widths = [T.kernel_dims(c)[5] for c in T.SMALL.values()]
    assert any(w < 24 for w in widths) and any(w >= 24 for w in widths)
    assert any(T.kernel_dims(c)[5] < 24 and T.kernel_dims(c)[5] % 4 != 0 for c in T.SMALL.values())      # the scalar-store path at XB = 16
    assert {c.form for c in T.SMALL.values()} == {"conv", "pool", "dgrad", "strip", "strip_prepare"}
    assert T.SMALL["dgrad"].signed and T.SMALL["strip"].signed and not T.SMALL["pool"].signed


def test_grid_lists():
    for c in T.SMALL.values():
        gs = T.grids(c)
        assert {1, 2, 3, 5, 8, 9, c.units - 1, c.units} == set(gs) and len(gs) == 8
        assert all(1 <= g <= c.units for g in gs)
        n = ncg(c)
        assert any(math.gcd(g, n) == 1 for g in gs) and any(g % n == 0 for g in gs), c.name
        assert any(g % 8 == 1 for g in gs if g > 8)                        # rem = 1 in zw_xcd_contiguous
        assert set(T.BOUND_GRIDS) <= set(gs)
        # G = units - 1: exactly one workgroup has two units
        lens = sorted(len(w) for w in T.walk(c.units, c.units - 1))
        assert lens[-1] == 2 and lens[-2] == 1


def test_release_cases_walk_three_units_unevenly():
    ragged = 0
    for c in T.RELEASE.values():
        assert c.units > 512
        rounds = cdiv(c.units, T.CUS)
        assert rounds >= 3
        grid = T.stock_grid(c.units)
        assert grid == cdiv(c.units, rounds) <= T.CUS
        ragged += c.units % grid != 0
        lens = {len(w) for w in T.walk(c.units, grid)}
        assert max(lens) == rounds and min(lens) >= rounds - 1
    assert ragged >= 1
    assert any(c.form == "pool" for c in T.RELEASE.values()) and any(c.form == "conv" for c in T.RELEASE.values())
    B, cin, cout, D, H, W = T.RELEASE["release_pool"].shape
    assert D % 2 == 0 and H % 2 == 0 and W % 2 == 0


def test_integer_exactness_obligation():
    for c in T.CASES.values():
        assert 3 * T.exact_half_units(c) < 2 ** 24, c.name                  # (x 3: the Winograd-z combination of three M_k)
        o = T.integer_operands(c)
        a, w = o["a"], o["w"]
        if c.form in ("strip", "strip_prepare"):
            a = a / T.window_powers(a.shape[0]).view(-1, 1, 1, 1, 1)
        assert float(a.abs().max()) == 7 and float(w.abs().max()) == 3 and bool((a == a.round()).all()) and bool((w == w.round()).all())
        assert (float(a.min()) < 0) == c.signed
        sc, sh = o["scale"], o["shift"]
        assert bool((sc.log2() == sc.log2().round()).all()) and bool((sh == sh.round()).all())
        assert sc.numel() == T.kernel_dims(c)[2]


def test_cost_cap():
    for c in T.SMALL.values():
        assert T.flop(c) <= T.CAP_FLOP, (c.name, T.flop(c))
    for c in T.RELEASE.values():
        assert T.flop(c) <= T.CAP_FLOP_RELEASE, (c.name, T.flop(c))


def test_the_walk_visits_every_unit_exactly_once():
    pairs = {(c.units, g) for c in T.SMALL.values() for g in T.grids(c)}
    pairs |= {(c.units, T.stock_grid(c.units)) for c in T.RELEASE.values()} | {(c.units, T.CUS) for c in T.RELEASE.values()}
    pairs |= {(u, g) for u in range(1, 71) for g in range(1, u + 1)}
    for units, grid in sorted(pairs):
        w = T.walk(units, grid)
        assert sorted(T.xcd_contiguous(b, grid) for b in range(grid)) == list(range(grid)), (units, grid)      # l0 is a permutation
        seen = sorted(u for ws in w for u in ws)
        assert seen == list(range(units)), (units, grid)
        assert all(len(ws) >= 1 for ws in w) and max(map(len, w)) - min(map(len, w)) <= 1, (units, grid)
        assert all(b - a == grid for ws in w for a, b in zip(ws, ws[1:]))


def test_unit_of_names_the_walk_position():
    c = T.SMALL["xb32"]                                                    # (2, 48, 70, 3, 5, 37): ncg 2, tiles 2 x 2 x 2
    assert T.unit_of(c, (0, 0, 0, 0, 0)) == 0 and T.unit_of(c, (0, 64, 0, 0, 0)) == 1 and T.unit_of(c, (0, 0, 0, 0, 32)) == 2
    assert T.unit_of(c, (0, 0, 0, 4, 0)) == 4 and T.unit_of(c, (0, 0, 2, 0, 0)) == 8 and T.unit_of(c, (1, 69, 2, 4, 36)) == 31
    c = T.SMALL["xb16"]
    assert T.unit_of(c, (1, 95, 2, 8, 19)) == 31 and T.unit_of(c, (0, 0, 0, 7, 15)) == 0


def test_the_release_library_refuses_the_grid_override(L):
    v = C.c_int(0)
    assert L.m3d_tuning_build() == 0
    assert L.m3d_set_option(b"tune_zw_grid", 4) == M3D_EUNSUPPORTED
    assert L.m3d_get_option(b"tune_zw_grid", C.byref(v)) == 0 and v.value == -1
