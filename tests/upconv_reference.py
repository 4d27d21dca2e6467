"""ConvTranspose3d(kernel 2, stride 2, padding 0) (+ ReLU) and its gradients restated in fp64 with einsum, with the sum of absolute terms
A_e of every output element, and the error bound the library states for its kernels (include/m3d.h, "Mask-head up-conv"):

    y [r,co,2z+a,2y+b,2x+c] = bias[co] + sum_ci x[r,ci,z,y,x] W[ci,co,a,b,c]               then ReLU if relu
    g = gy [y > 0] if relu else gy                                                          (y: the forward's own output)
    gx[r,ci,z,y,x]          = sum_{co,a,b,c} g[r,co,2z+a,2y+b,2x+c] W[ci,co,a,b,c]          (reduction 8 Cout)
    gW[ci,co,a,b,c]         = sum_{r,z,y,x}  x[r,ci,z,y,x] g[r,co,2z+a,2y+b,2x+c]           (reduction R D H W)
    gb[co]                  = sum g[r,co,.,.,.]                                             (8 R D H W terms)

    |out - out64| <= gamma_n A_e + 2^-24 |out64|,  n = reduction length + partials added (the forward: + 1 for the bias),
    gamma_n = n 2^-24 / (1 - n 2^-24): it holds for ANY order of a fp32 summation of n terms whose products are rounded once."""
import numpy as np

# (R, Cin, Cout, D, H, W): the degenerate case; everything ragged; the MaskHead test's size; channels crossing the 32- and 64-wide tiles
# and a row longer than one 32-lane tile; the shipped channel count
SHAPES = [(1, 1, 1, 1, 1, 1), (3, 5, 3, 2, 3, 5), (2, 16, 16, 7, 7, 7), (2, 40, 72, 3, 4, 33), (1, 256, 256, 7, 7, 7)]
U = 2.0 ** -24


def shuffled(g):
    """[R,Co,2D,2H,2W] -> [R,Co,2,2,2,D,H,W] with [r,co,a,b,c,z,y,x] = g[r,co,2z+a,2y+b,2x+c]"""
    R, Co, D2, H2, W2 = g.shape
    return g.reshape(R, Co, D2 // 2, 2, H2 // 2, 2, W2 // 2, 2).transpose(0, 1, 3, 5, 7, 2, 4, 6)


def unshuffled(t):
    R, Co, _, _, _, D, H, W = t.shape
    return np.ascontiguousarray(t.transpose(0, 1, 5, 2, 6, 3, 7, 4)).reshape(R, Co, 2 * D, 2 * H, 2 * W)


def forward(x, w, bias=None, relu=False):
    """-> (y64 [R,Co,2D,2H,2W], A [same]): A = sum_ci |x| |W| + |bias|"""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    t = np.einsum("rizyx,ioabc->roabczyx", x, w, optimize=True)
    A = np.einsum("rizyx,ioabc->roabczyx", np.abs(x), np.abs(w), optimize=True)
    if bias is not None:
        b = np.asarray(bias, np.float64)[None, :, None, None, None, None, None, None]
        t, A = t + b, A + np.abs(b)
    y = unshuffled(t)
    return (np.maximum(y, 0.0) if relu else y), unshuffled(A)


def masked(gy, y_mask=None):
    gy = np.asarray(gy, np.float64)
    return gy if y_mask is None else gy * (np.asarray(y_mask) > 0)


def dgrad(gy, w, y_mask=None):
    """-> (gx64 [R,Ci,D,H,W], A)"""
    G, w = shuffled(masked(gy, y_mask)), np.asarray(w, np.float64)
    return (np.einsum("roabczyx,ioabc->rizyx", G, w, optimize=True),
            np.einsum("roabczyx,ioabc->rizyx", np.abs(G), np.abs(w), optimize=True))


def wgrad(gy, x, y_mask=None):
    """-> (gw64 [Ci,Co,2,2,2], A_w, gb64 [Co], A_b)"""
    G, x = shuffled(masked(gy, y_mask)), np.asarray(x, np.float64)
    return (np.einsum("rizyx,roabczyx->ioabc", x, G, optimize=True), np.einsum("rizyx,roabczyx->ioabc", np.abs(x), np.abs(G), optimize=True),
            G.sum(axis=(0, 2, 3, 4, 5, 6, 7)), np.abs(G).sum(axis=(0, 2, 3, 4, 5, 6, 7)))


def gamma(n):
    return n * U / (1.0 - n * U)


def bound(out64, A, n):
    return gamma(n) * A + U * np.abs(out64)


def worst_ratio(got, out64, A, n):
    """largest err / bound over the elements; an element whose bound is 0 must be exact (ratio 0, or inf if it is not)"""
    err, b = np.abs(np.asarray(got, np.float64) - out64), bound(out64, A, n)
    r = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1.0))
    r = np.where((b == 0) & (err > 0), np.inf, r)
    return float(r.max()) if r.size else 0.0


def lengths(R, Cin, Cout, D, H, W):
    """reduction lengths of forward, dgrad, wgrad, gb"""
    return {"forward": Cin, "dgrad": 8 * Cout, "wgrad": R * D * H * W, "gb": 8 * R * D * H * W}


def case(shape, kind, seed=0):
    """x, w, bias, gy as float32 arrays: kind "int" = integers in [-4, 4] (every sum exact in fp32), "randn" = normal"""
    R, Cin, Cout, D, H, W = shape
    g = np.random.default_rng([seed, R, Cin, Cout, D, H, W])
    shapes = ((R, Cin, D, H, W), (Cin, Cout, 2, 2, 2), (Cout,), (R, Cout, 2 * D, 2 * H, 2 * W))
    if kind == "int":
        return tuple(g.integers(-4, 5, s).astype(np.float32) for s in shapes)
    return tuple(g.standard_normal(s).astype(np.float32) for s in shapes)
