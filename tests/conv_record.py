"""The recording double of the library that the launch-record tests (test_conv_dispatch.py, test_conv_train_dispatch.py) run the real
dispatch code against, on meta tensors: pure host queries reach the real libm3d.so and are counted, every other entry point is not
called but written down (its name, every integer argument, null / non-null per pointer).

And what the three training-dispatch modules (test_conv_train_dispatch*.py) share: the grid of the five older switches that
tests/golden/conv_train_dispatch.json.gz was recorded over, the key of a setting in that record, and the meta tensors they call on."""
import ctypes as C
import itertools
import types

import torch

# ----------------------------------------------------------------------------- the training-dispatch grid
TRAIN = (("fp32", None), ("f16x2", None), ("f16x2", 0))          # set_conv_train(mode, min_units)
NARROW = ((False, None), (True, None), (True, 0))                # set_conv_train_narrow(on, min_units)
WGRAD = ("fp32", "f16x2")
WGRAD_NARROW = (False, True)
DILATED = ("torch", "m3d")
SETTINGS = tuple(itertools.product(TRAIN, NARROW, WGRAD, WGRAD_NARROW, DILATED))
DEFAULT = (("fp32", None), (False, None), "fp32", False, "torch")
# (x, weight, bias) requires_grad; None: the layer has no bias
NEEDS = {"xwb": (True, True, True), "-wb": (False, True, True), "x--": (True, False, False), "xw.": (True, True, None)}


def setting_key(setting):
    """the golden records are indexed by this string"""
    (mode, mu), (narrow, nmu), wgrad, wn, dil = setting
    return "train=%s/%s narrow=%s/%s wgrad=%s wn=%d dil=%s" % (mode, mu, int(narrow), nmu, wgrad, wn, dil)


def train_setting(cp, setting):
    """the grid point as a conv_plan.TrainSetting"""
    (mode, mu), (narrow, nmu), wgrad, wn, dil = setting
    return cp.TrainSetting(train=mode, min_units=mu, narrow=(cp.ZN_MIN_UNITS if nmu is None else nmu) if narrow else None,
                           wgrad=wgrad, wgrad_narrow=wn, dilated=dil)


def meta(shape, grad, contiguous=True):
    if contiguous:
        t = torch.empty(shape, device="meta")
    else:                                                       # channels innermost
        B, C_, D, H, W = shape
        t = torch.empty_strided(shape, (C_ * D * H * W, 1, H * W * C_, W * C_, C_), device="meta")
        assert not t.is_contiguous()
    return t.as_subclass(CudaMeta).requires_grad_(bool(grad))


# ----------------------------------------------------------------------------- the recording double
PURE = ("_supported", "_score", "_bytes", "_family", "_units", "_plan", "_geometry", "_max_boxes", "_version", "_tuning_build")


class CudaMeta(torch.Tensor):
    """a meta tensor that says it is on the GPU (PackedConv3d.__call__ asserts it of scale and shift)"""
    is_cuda = property(lambda self: True)


def _arg(v):
    if v is None:
        return "null"
    if isinstance(v, C.c_void_p):
        return "ptr" if v.value else "null"
    if type(v).__name__ == "CArgObject":          # C.byref(...): an in / out scalar
        return "ref"
    return int(getattr(v, "value", v))


class Recorder:
    """stands in for the ctypes library object: pure queries reach the real one and are counted, launches are written down"""

    def __init__(self, real):
        self.real, self.launches, self.queries = real, [], 0

    def __getattr__(self, name):
        if name.endswith(PURE):
            fn = getattr(self.real, name)

            def query(*a):
                self.queries += 1
                return fn(*a)
            return query

        def launch(*a):
            self.launches.append([name] + [_arg(v) for v in a])
            return 0
        return launch

    def take(self):
        out = (self.launches, self.queries)
        self.launches, self.queries = [], 0
        return out


def install(mp):
    """the doubles at the ops / library boundary, through the MonkeyPatch `mp`"""
    import __graft_entry__ as g
    g.build()
    from m3d import ops, _lib
    rec = Recorder(_lib.lib())
    mp.setattr(ops, "lib", lambda: rec)
    mp.setattr(ops, "_need_gpu", lambda *ts: None)
    mp.setattr(ops, "_stream", lambda: C.c_void_p(0))
    mp.setattr(ops, "_ptr", lambda t: C.c_void_p(0 if t is None else 1))
    mp.setattr(torch.cuda, "current_stream", lambda *a, **k: types.SimpleNamespace(cuda_stream=0))
    return rec
