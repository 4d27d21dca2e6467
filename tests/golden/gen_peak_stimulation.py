"""Writes tests/golden/peak_stimulation.npz: the reference's own peak_stimulation_3d (lib/prm/peak_stimulation_3d.py:6-52) and its
backward, run on torch-CPU, on small inputs with heavy ties, NaNs, a plateau, every filter and windows 1 / 3 / 5.

Runs only where a checkout of the reference is at hand (its path is the first argument, default /root/reference); the file is loaded
in place with importlib - nothing of it is copied.  Every input is a multiple of 2^-6 (mostly of 1/4), so every fp32 sum the reference
takes is exact in any order and the recorded thresholds and aggregations can be compared exactly.

Per case NAME the archive holds NAME_x, NAME_win, NAME_filter ('none' | 'median' | 'mean' | 'max' | 'const' | 'tensor'), NAME_value (the
constant), NAME_thresh [B,C] (what the filter evaluated to; -inf without one), NAME_peaks int64 [N,5], NAME_agg [B,C], NAME_gy [B,C],
NAME_gx; `names` lists the cases.

win 1: the reference's function cannot run it - its `element_map[..., offset:-offset]` (:18) is an empty slice for offset 0 and the
comparison at :25 raises.  The two win-1 cases are therefore recorded from the same torch statements (:15-39) written out below with that
one slice left out, which is what the statements mean for offset 0: every voxel is the arg-max of its own window."""
import importlib.util
import os
import sys

import numpy as np
import torch


def load_reference(root):
    spec = importlib.util.spec_from_file_location("ref_peak_stimulation_3d", os.path.join(root, "lib", "prm", "peak_stimulation_3d.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def win1_statements(x, filt):
    """peak_stimulation_3d.py:15-39 for win_size 1 (offset 0, no padding, the slice at :18 dropped) -> peak list, aggregation and the
    float peak map its backward multiplies the gradient with (:47)."""
    b, c, s, h, w = x.shape
    element_map = torch.arange(0, s * h * w).long().view(1, 1, s, h, w)
    _, indices = torch.nn.functional.max_pool3d(x, kernel_size=1, stride=1, return_indices=True)
    peak_map = indices == element_map
    if filt:
        peak_map = peak_map & (x >= filt(x))
    peak_list = torch.nonzero(peak_map)
    pm = peak_map.float()
    return peak_list, (x * pm).view(b, c, -1).sum(2) / pm.view(b, c, -1).sum(2), pm


def flat_filter(fn):
    def f(t):
        b, c = t.shape[:2]
        return fn(t.reshape(b, c, -1)).contiguous().view(b, c, 1, 1, 1)
    return f


FILTERS = {
    "median": flat_filter(lambda v: torch.median(v, dim=2)[0]),           # peak_response_mapping_3d.py:46-49
    "mean": flat_filter(lambda v: torch.mean(v, dim=2)),                  # :52-55
    "max": flat_filter(lambda v: torch.max(v, dim=2)[0]),                 # :58-61
}


def main():
    root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    ref = load_reference(root)
    g = torch.Generator().manual_seed(20261019)

    def quarters(shape):
        return torch.randint(0, 4, shape, generator=g).float() / 4

    def sixtyfourths(shape):
        return torch.randint(-32, 64, shape, generator=g).float() / 64

    base = quarters((2, 2, 5, 6, 7))                                       # n = 210, even
    odd = quarters((1, 2, 3, 5, 7))                                        # n = 105, odd
    nan2 = base.clone()
    nan2[0, 0, 2, 2, 2] = float("nan")
    nan2[0, 0, 2, 3, 3] = float("nan")
    fine = sixtyfourths((2, 3, 4, 5, 6))
    half_max = flat_filter(lambda v: torch.max(v, dim=2)[0] * 0.5)         # a caller's own callable: half the channel maximum
    cases = [
        ("ties_w3", base, 3, "none", None),
        ("ties_w5", base, 5, "none", None),
        ("ties_w3_median_even", base, 3, "median", None),
        ("ties_w5_median_odd", odd, 5, "median", None),
        ("nan2_w3", nan2, 3, "none", None),
        ("nan2_w3_median", nan2, 3, "median", None),
        ("nan2_w3_const", nan2, 3, "const", 0.5),
        ("ones_w3", torch.ones((2, 2, 5, 6, 7)), 3, "none", None),
        ("ones_w5_median", torch.ones((1, 2, 3, 5, 7)), 5, "median", None),
        ("const_above", base, 3, "const", 10.0),
        ("const_half", base, 3, "const", 0.5),
        ("win1", odd, 1, "none", None),
        ("win1_mean", fine, 1, "mean", None),
        ("mean_w3", fine, 3, "mean", None),
        ("max_w3", base, 3, "max", None),
        ("callable_w3", fine, 3, "tensor", half_max),
    ]
    out = {"names": np.array([c[0] for c in cases])}
    for name, x, win, kind, arg in cases:
        if kind == "none":
            filt = None
        elif kind == "const":
            filt = (lambda v: (lambda t: v))(float(arg))                    # peak_response_mapping_3d.py:40-41
        elif kind == "tensor":
            filt = arg
        else:
            filt = FILTERS[kind]
        xin = x.clone().requires_grad_(True)
        b, c = x.shape[:2]
        gy = torch.randint(-8, 9, (b, c), generator=g).float() / 8
        if win > 1:
            peaks, agg = ref.peak_stimulation_3d(xin, True, win, filt)
            (gx,) = torch.autograd.grad(agg, xin, gy)                       # the function's own backward (:43-48)
        else:
            peaks, agg, pm = win1_statements(x, filt)
            gx = pm * gy.view(b, c, 1, 1, 1)                                # :47
        if kind == "none":
            thr = torch.full((b, c), float("-inf"))
        elif kind == "const":
            thr = torch.full((b, c), float(arg))
        else:
            thr = filt(x).reshape(b, c)
        out[name + "_x"] = x.numpy().astype(np.float32)
        out[name + "_win"] = np.int32(win)
        out[name + "_filter"] = np.array(kind)
        out[name + "_value"] = np.float32(arg if kind == "const" else 0.0)
        out[name + "_thresh"] = thr.numpy().astype(np.float32)
        out[name + "_peaks"] = peaks.numpy().astype(np.int64)
        out[name + "_agg"] = agg.detach().numpy().astype(np.float32)
        out[name + "_gy"] = gy.numpy().astype(np.float32)
        out[name + "_gx"] = gx.numpy().astype(np.float32)
        print("%-22s win %d %-6s peaks %4d" % (name, win, kind, peaks.shape[0]))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "peak_stimulation.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, torch %s)" % (path, os.path.getsize(path), torch.__version__))


if __name__ == "__main__":
    main()
