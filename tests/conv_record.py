"""The recording double of the library that the launch-record tests (test_conv_dispatch.py, test_conv_train_dispatch.py) run the real
dispatch code against, on meta tensors: pure host queries reach the real libm3d.so and are counted, every other entry point is not
called but written down (its name, every integer argument, null / non-null per pointer)."""
import ctypes as C
import types

import torch

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
