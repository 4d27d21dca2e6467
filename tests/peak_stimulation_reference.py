"""NumPy restatement of the peak stimulation contract (lib/prm/peak_stimulation_3d.py:6-52; include/m3d.h, m3d_peak_stimulation3d).

Input x fp32 [B,C,S,H,W], win odd, o = win // 2.
  peak map     v is a peak iff it is the arg-max of its window [z-o,z+o] x [y-o,y+o] x [x-o,x+o] clipped to the volume; ties go to the
               first maximum in raster order; a NaN beats everything, among NaNs the last in raster order wins.  Written as the maximum
               of one key per voxel, (value, descending raster index), for a NaN (largest, ascending raster index), taken over x, y, z.
  filter       a peak must also satisfy x >= thr[b,c] (false for a NaN on either side).  'median': the element of rank (n-1)//2
               ascending, NaN if the channel holds one, -0.0 == +0.0; 'mean': the fp64 sum / n rounded to fp32 once; 'max'; a number; a
               [B,C] array.  Without a filter the threshold output is -inf.
  peak list    rows (b,c,z,y,x) in raster order over the whole tensor (np.argwhere).
  aggregation  (float32)(sum of x * peak over the channel, fp64 in raster order, / count); count == 0 gives NaN.
  backward     gx = peak_map * gy[b,c].
"""
import numpy as np

NAN_ORD = np.uint64(0xFFFFFFFF)


def ordered(x):
    """Monotone uint32 image of fp32 values: -inf lowest, +inf = 0xFF800000, -0.0 == +0.0, every NaN 0xFFFFFFFF."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    o = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    o[np.isnan(x)] = 0xFFFFFFFF
    return o


def keys(x):
    """uint64 key of every voxel of x [B,C,S,H,W]; the raster index is the voxel's index inside its (b,c) volume."""
    B, C, S, H, W = x.shape
    idx = np.arange(S * H * W, dtype=np.uint64).reshape(1, 1, S, H, W)
    o = ordered(x).astype(np.uint64)
    low = np.where(o == NAN_ORD, idx, np.uint64(0xFFFFFFFF) - idx)
    return (o << np.uint64(32)) | low


def window_max(k, o):
    """Maximum of k over the clipped (2o+1)^3 window around every voxel, axis by axis."""
    for axis in (4, 3, 2):
        src = k
        out = src.copy()
        n = src.shape[axis]
        for d in range(1, min(o, n - 1) + 1):
            a = [slice(None)] * 5
            b = [slice(None)] * 5
            a[axis], b[axis] = slice(0, n - d), slice(d, n)
            a, b = tuple(a), tuple(b)
            out[a] = np.maximum(out[a], src[b])
            out[b] = np.maximum(out[b], src[a])
        k = out
    return k


def local_maxima(x, win):
    assert win % 2 == 1 and win >= 1
    k = keys(x)
    return window_max(k, win // 2) == k


def serial_sum64(v):
    """fp64 sum of v along the last axis in index order (np.sum adds pairwise; cumsum does not)."""
    v = np.asarray(v, dtype=np.float64)
    if v.shape[-1] == 0:
        return np.zeros(v.shape[:-1], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.cumsum(v, axis=-1)[..., -1]


def thresholds(x, filt):
    """fp32 [B,C] for filt = None | 'median' | 'mean' | 'max' | number | array of B*C elements."""
    B, C = x.shape[:2]
    flat = np.ascontiguousarray(x, dtype=np.float32).reshape(B, C, -1)
    n = flat.shape[2]
    if filt is None:
        return np.full((B, C), -np.inf, np.float32)
    if isinstance(filt, str):
        if filt == "median":
            s = np.sort(flat + np.float32(0.0), axis=2)            # np.sort puts NaN last; x + 0.0 turns -0.0 into +0.0
            out = s[:, :, (n - 1) // 2].copy()
            out[np.isnan(flat).any(2)] = np.nan
            return out.astype(np.float32)
        if filt == "mean":
            return (serial_sum64(flat) / np.float64(n)).astype(np.float32)
        if filt == "max":
            with np.errstate(invalid="ignore"):
                return flat.max(2).astype(np.float32)             # np.max propagates NaN, as torch.max does
        raise ValueError(filt)
    if np.isscalar(filt):
        return np.full((B, C), np.float32(filt), np.float32)
    return np.asarray(filt, dtype=np.float32).reshape(B, C).copy()


def peak_stimulation(x, win=3, filt=None, thresh=None):
    """-> dict(peak_map bool [B,C,S,H,W], peaks int64 [N,5], thresh fp32 [B,C], agg fp32 [B,C]).  `thresh` (fp32 [B,C]) overrides the
    thresholds of `filt` - the filter is then applied with exactly these values."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, C = x.shape[:2]
    pm = local_maxima(x, win)
    thr = thresholds(x, filt) if thresh is None else np.asarray(thresh, np.float32).reshape(B, C)
    if filt is not None or thresh is not None:
        with np.errstate(invalid="ignore"):
            pm = pm & (x >= thr[:, :, None, None, None])
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (x * pm.astype(np.float32)).reshape(B, C, -1)       # input * peak_map: 0 * NaN is NaN here as well
        cnt = pm.reshape(B, C, -1).sum(2).astype(np.float64)
        agg = (serial_sum64(prod) / cnt).astype(np.float32)
    return dict(peak_map=pm, peaks=np.argwhere(pm).astype(np.int64).reshape(-1, 5), thresh=thr, agg=agg)


def backward(peak_map, gy):
    B, C = peak_map.shape[:2]
    with np.errstate(invalid="ignore"):
        return peak_map.astype(np.float32) * np.asarray(gy, np.float32).reshape(B, C, 1, 1, 1)
