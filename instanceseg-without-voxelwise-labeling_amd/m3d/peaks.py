"""Peak stimulation (lib/prm/peak_stimulation_3d.py:6-52) on csrc/peak_stim.hip: the local maxima of a class response map, their
per-channel filter, the ordered peak list and the masked-mean aggregation PRM trains its classification branch through.

  peak_stimulation_3d(input, return_aggregation=True, win_size=3, peak_filter=None)   the reference's signature and returns
  peak_stimulation_3d_dev(input, win_size=3, peak_filter=None, cap=None, ...)         no host synchronisation: device tensors only

The contract (tie and NaN rule, thresholds, order of the list, aggregation) is stated at m3d_peak_stimulation3d in include/m3d.h and
in DESIGN.md, "Peak stimulation".  There is no CPU path."""
import ctypes as C
import numbers

import numpy as np
import torch

from ._lib import lib, check, M3DError
from .ops import _ptr, _stream, _need_gpu, _peak_pool

__all__ = ["peak_stimulation_3d", "peak_stimulation_3d_dev", "PeakStimulation", "DEFAULT_PEAK_CAP"]

FILTER_NONE, FILTER_MEDIAN, FILTER_MEAN, FILTER_MAX, FILTER_CONST, FILTER_TENSOR = range(6)
_NAMED = {"median": FILTER_MEDIAN, "mean": FILTER_MEAN, "max": FILTER_MAX}
DEFAULT_PEAK_CAP = 1 << 20


def _resolve_filter(input, peak_filter):
    """peak_filter -> (kind, constant, thresholds [B*C] on the device or None).  A callable is what the reference passes (:28-29): it is
    called on `input`; a [B,C,1,1,1] (any shape of B*C elements) tensor result is the threshold tensor, a number the constant."""
    if callable(peak_filter):
        peak_filter = peak_filter(input)
        if peak_filter is None:
            raise M3DError("peak_filter(input) returned None")
    if peak_filter is None:
        return FILTER_NONE, 0.0, None
    if isinstance(peak_filter, str):
        if peak_filter not in _NAMED:
            raise ValueError("peak_filter %r: expected 'median', 'mean', 'max', a number, a callable or None" % (peak_filter,))
        return _NAMED[peak_filter], 0.0, None
    if torch.is_tensor(peak_filter):
        if peak_filter.numel() != input.shape[0] * input.shape[1]:
            raise ValueError("peak_filter tensor must hold one threshold per (batch, channel): %d elements, got %s"
                             % (input.shape[0] * input.shape[1], tuple(peak_filter.shape)))
        _need_gpu(peak_filter)
        return FILTER_TENSOR, 0.0, peak_filter.detach().to(torch.float32).reshape(-1).contiguous()
    if isinstance(peak_filter, numbers.Real) and not isinstance(peak_filter, bool):
        return FILTER_CONST, float(peak_filter), None
    raise ValueError("peak_filter %r: expected 'median', 'mean', 'max', a number, a callable or None" % (peak_filter,))


def _check_input(input, win_size):
    if not torch.is_tensor(input) or input.dim() != 5:
        raise ValueError("peak stimulation takes a [B,C,S,H,W] tensor")
    _need_gpu(input)
    if input.dtype != torch.float32:
        raise ValueError("peak stimulation takes an fp32 tensor, got %s" % input.dtype)
    if int(win_size) != win_size or win_size < 1 or win_size % 2 != 1:
        raise ValueError("Window size for peak finding must be odd.")                                     # :13


def peak_stimulation_3d_dev(input, win_size=3, peak_filter=None, cap=None, aggregation=True, mirror=False):
    """The op without a host synchronisation.  input fp32 CUDA [B,C,S,H,W] -> dict of device tensors: peaks int32 [cap,5] = rows
    (b,c,z,y,x) in raster order (rows at and beyond num are not written), num int64 [1] = the true peak count (it may exceed cap),
    thresh fp32 [B,C], agg fp32 [B,C] (None with aggregation=False), peak_map uint8 [B,C,S,H,W].  cap defaults to the element count.
    mirror=True adds `host_num` (a pinned int64 [1] the same launch writes), `event` (recorded behind it) and `release()` (hands the
    pinned buffer back; call it after reading)."""
    _check_input(input, win_size)
    x = input.detach()
    x = x if x.is_contiguous() else x.contiguous()
    B, Cn, S, H, W = (int(v) for v in x.shape)
    total = x.numel()
    cap = total if cap is None else int(cap)
    if cap < 0 or cap >= 1 << 31:
        raise ValueError("cap must be in [0, 2^31)")
    kind, value, thr_in = _resolve_filter(x, peak_filter)
    dev = x.device
    peaks = torch.empty((cap, 5), dtype=torch.int32, device=dev)
    num = torch.zeros((1,), dtype=torch.int64, device=dev)
    thresh = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    agg = torch.empty((B, Cn), dtype=torch.float32, device=dev) if aggregation else None
    peak_map = torch.empty(x.shape, dtype=torch.uint8, device=dev)
    out = dict(peaks=peaks, num=num, thresh=thresh, agg=agg, peak_map=peak_map)
    L = lib()
    ws_bytes = int(L.m3d_peak_stimulation3d_workspace_bytes(B, Cn, S, H, W, int(win_size))) if B * Cn else 0
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    buf = _peak_pool.take(64) if mirror else None
    if buf is not None:
        buf.numpy()[:8].view(np.int64)[0] = 0                     # B * C == 0: the call writes nothing
    with torch.cuda.device(dev):
        check(L.m3d_peak_stimulation3d(_ptr(x), B, Cn, S, H, W, int(win_size), kind, C.c_float(np.float32(value)), _ptr(thr_in),
                                       _ptr(peak_map), _ptr(peaks), cap, _ptr(num), C.c_void_p(buf.data_ptr() if mirror else 0),
                                       _ptr(thresh), _ptr(agg), _ptr(ws), C.c_size_t(ws_bytes), _stream()), "peak_stimulation3d")
        if mirror:
            ev = torch.cuda.Event()
            ev.record()
            out.update(host_num=buf.numpy()[:8].view(np.int64), event=ev, release=lambda: _peak_pool.give(buf))
    return out


def _peaks_sync(input, win_size, peak_filter, aggregation):
    """The op with its one host read (the count, through the pinned mirror and an event) -> (peaks int32 [N,5], dev dict).  The list
    buffer holds min(elements, 2^20) rows; a map with more peaks than that runs once more with the true count."""
    cap = min(input.numel(), DEFAULT_PEAK_CAP)
    for _ in range(2):
        out = peak_stimulation_3d_dev(input, win_size, peak_filter, cap=cap, aggregation=aggregation, mirror=True)
        out["event"].synchronize()
        n = int(out["host_num"][0])
        out["release"]()
        if n <= cap:
            return out["peaks"][:n], out
        cap = n
    raise M3DError("peak stimulation: the peak count changed between two runs on the same input")


class PeakStimulation(torch.autograd.Function):
    """peak_stimulation_3d.py:6-48."""

    @staticmethod
    def forward(ctx, input, return_aggregation, win_size, peak_filter):
        peaks, out = _peaks_sync(input, win_size, peak_filter, bool(return_aggregation))
        peak_list = peaks.to(torch.int64)                                                                 # torch.nonzero's dtype (:31)
        ctx.mark_non_differentiable(peak_list)
        if return_aggregation:
            ctx.peak_map = out["peak_map"]
            return peak_list, out["agg"]
        return peak_list

    @staticmethod
    def backward(ctx, grad_peak_list, grad_output=None):
        pm = ctx.peak_map
        B, Cn, S, H, W = (int(v) for v in pm.shape)
        if grad_output is None:
            return torch.zeros(pm.shape, dtype=torch.float32, device=pm.device), None, None, None
        gy = grad_output.detach().to(torch.float32).reshape(-1).contiguous()
        if gy.numel() != B * Cn:
            raise ValueError("peak stimulation backward: the aggregation's gradient must be [B,C]")
        gx = torch.empty(pm.shape, dtype=torch.float32, device=pm.device)
        with torch.cuda.device(pm.device):
            check(lib().m3d_peak_stimulation3d_backward(_ptr(pm), _ptr(gy), B, Cn, S, H, W, _ptr(gx), _stream()), "peak_stimulation3d_backward")
        return gx, None, None, None


def peak_stimulation_3d(input, return_aggregation=True, win_size=3, peak_filter=None):
    """peak_stimulation_3d.py:51-52: (peak_list int64 [N,5], aggregation [B,C]) or, with return_aggregation=False, peak_list.
    peak_filter: 'median' | 'mean' | 'max', a number (that constant), None, or a callable as the reference passes (called on `input`; its
    [B,C,1,1,1] result is the threshold tensor).  One host wait, for the peak count."""
    _check_input(input, win_size)
    return PeakStimulation.apply(input, return_aggregation, win_size, peak_filter)
