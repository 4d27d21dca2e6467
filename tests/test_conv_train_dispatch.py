"""CPU: which library entry points a training conv launches, forward and backward, pinned against a launch record.

m3d.compat.conv3d and torch.autograd.grad run on meta tensors against the recording double of the library (tests/conv_record.py): the
pure host queries go through to the real libm3d.so and are counted, every other entry point is written down with its integer arguments
and null / non-null per pointer.  A call that falls through to torch's conv3d is recorded as "torch" (a stand-in for
compat._orig_conv3d) and its gradient is not taken.  tests/golden/conv_train_dispatch.json.gz holds what the commit before the
training plan (conv_plan.plan_train_conv) launched over the grid below (tests/golden/gen_conv_train_dispatch.py writes it): the product
of every combination of the five switches, four needs_input_grad patterns and the layers at which a route can change.  The launches,
their arguments and their order must not move, and a call on a shape seen before may not ask the library more than it did.

The "flip" records turn every switch over between the forward and the backward of a call: they pin WHEN each switch is read (the train
mode, its threshold, the narrow switch and the dilated mode at forward time; the two wgrad switches when the backward runs).
test_each_field_is_read_when_its_table_says does the same for every field of conv_plan.TrainSetting, one at a time, against
conv_plan.FORWARD_FIELDS / BACKWARD_FIELDS.
"""
import gzip
import inspect
import itertools
import json
import os
import re

import pytest
import torch

from conv_record import DEFAULT, DILATED, NEEDS, SETTINGS, WGRAD, CudaMeta, install, meta, setting_key, train_setting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_train_dispatch.json.gz")

# name: (x shape, (cout, cin, k), dilation, padding, contiguous x)
LAYERS = {
    "stem 1-32 k5": ((2, 1, 17, 33, 63), (32, 1, 5), 1, 2, True),
    "body 32-64": ((2, 32, 17, 33, 63), (64, 32, 3), 1, 1, True),
    "body 64-64": ((2, 64, 17, 33, 63), (64, 64, 3), 1, 1, True),
    "body 24-64": ((2, 24, 17, 33, 63), (64, 24, 3), 1, 1, True),             # cin no multiple of 16
    "body 64-130": ((2, 64, 17, 33, 63), (130, 64, 3), 1, 1, True),           # the dgrad has no f16x2 configuration
    "item 1GiB 16-32": ((1, 16, 64, 512, 512), (32, 16, 3), 1, 1, True),      # below ITEM_LIMIT
    "item 2GiB 16-32": ((1, 16, 128, 512, 512), (32, 16, 3), 1, 1, True),     # at it
    "work 2^27 128-256": ((1, 128, 16, 16, 16), (256, 128, 3), 1, 1, True),   # wgrad work exactly WGRAD_F16X2_MIN_WORK
    "work 2^26 128-256": ((1, 128, 8, 16, 16), (256, 128, 3), 1, 1, True),
    "k1 64-35": ((2, 64, 17, 33, 63), (35, 64, 1), 1, 0, True),
    "roi R4 32-64": ((4, 32, 7, 7, 7), (64, 32, 3), 1, 1, True),
    "roi R16 256-256": ((16, 256, 7, 7, 7), (256, 256, 3), 1, 1, True),       # 128 narrow units: ZN_MIN_UNITS
    "roi R15 256-256": ((15, 256, 7, 7, 7), (256, 256, 3), 1, 1, True),
    "roi R70 256-32": ((70, 256, 7, 7, 7), (32, 256, 3), 1, 1, True),
    "roi R4 32-64 strided": ((4, 32, 7, 7, 7), (64, 32, 3), 1, 1, False),
    "dil2 32-32": ((4, 32, 14, 14, 14), (32, 32, 3), 2, 2, True),
    "dil2 32-32 strided": ((4, 32, 14, 14, 14), (32, 32, 3), 2, 2, False),
    "dil3 32-32": ((4, 32, 14, 14, 14), (32, 32, 3), 3, 3, True),
    "pad0 32-32": ((4, 32, 14, 14, 14), (32, 32, 3), 1, 0, True),             # not a 'same' conv: torch
    "map W12 64-64": ((2, 64, 9, 10, 12), (64, 64, 3), 1, 1, True),
    "map W8 64-64": ((2, 64, 9, 10, 8), (64, 64, 3), 1, 1, True),
}
FLIP_LAYERS = ("body 64-64", "roi R16 256-256", "dil2 32-32", "map W8 64-64", "work 2^27 128-256")

def flipped(setting):
    """every switch turned over"""
    (mode, _), (narrow, _), wgrad, wn, dil = setting
    return (("fp32", None) if mode == "f16x2" else ("f16x2", 0), (False, None) if narrow else (True, 0),
            WGRAD[wgrad == "fp32"], not wn, DILATED[dil == "torch"])


def case_key(layer, needs, setting, flip=False):
    return "%s | %s | %s%s" % (layer, needs, setting_key(setting), " | flip" if flip else "")


def cases():
    for layer, needs, setting in itertools.product(LAYERS, NEEDS, SETTINGS):
        yield layer, needs, setting, False
    for layer, setting in itertools.product(FLIP_LAYERS, SETTINGS):
        yield layer, "xwb", setting, True


def apply_setting(compat, setting):
    train, narrow, wgrad, wn, dil = setting
    compat.set_conv_train(*train)
    compat.set_conv_train_narrow(*narrow)
    compat.set_conv_wgrad(wgrad)
    compat.set_conv_wgrad_narrow(wn)
    compat.set_conv_dilated(dil)


def run_case(compat, rec, layer, needs, setting, flip):
    """-> {"forward": launches | "torch", "backward": launches, "queries": n}: the second of two identical calls, which must launch alike"""
    xshape, (cout, cin, k), dilation, padding, contiguous = LAYERS[layer]
    gx, gw, gb = NEEDS[needs]
    out = None
    for _ in range(2):
        apply_setting(compat, setting)
        x, w = meta(xshape, gx, contiguous), meta((cout, cin, k, k, k), gw)
        b = None if gb is None else meta((cout,), gb)
        rec.take()
        y = compat.conv3d(x, w, b, 1, padding, dilation, 1)
        fwd, queries = rec.take()
        if isinstance(y, str):                                  # the stand-in for torch's conv3d
            assert not fwd
            got = {"forward": "torch"}
        else:
            assert tuple(y.shape) == (xshape[0], cout) + tuple(xshape[2:])
            if flip:
                apply_setting(compat, flipped(setting))
            gy = torch.empty(y.shape, device="meta").as_subclass(CudaMeta)
            grads = torch.autograd.grad(y, [t for t in (x, w, b) if t is not None and t.requires_grad], gy)
            assert all(g is not None for g in grads)
            bwd, q2 = rec.take()
            got = {"forward": fwd, "backward": bwd, "queries": queries + q2}
        assert out is None or {k_: v for k_, v in out.items() if k_ != "queries"} == {k_: v for k_, v in got.items() if k_ != "queries"}
        out = got
    return out


def record_all(mp):
    """the whole grid: {case_key: run_case}"""
    rec = install(mp)
    from m3d import compat
    mp.setattr(compat, "_orig_conv3d", lambda *a: "torch")
    out = {}
    try:
        for layer, needs, setting, flip in cases():
            out[case_key(layer, needs, setting, flip)] = run_case(compat, rec, layer, needs, setting, flip)
    finally:
        apply_setting(compat, DEFAULT)
    return json.loads(json.dumps(out))          # as the fixture reads back


@pytest.fixture(scope="module")
def recorded():
    with pytest.MonkeyPatch.context() as mp:
        return record_all(mp)


@pytest.fixture(scope="module")
def fixture():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def entry_names(record):
    if record["forward"] == "torch":
        return {"torch"}
    return {launch[0] for launch in record["forward"] + record["backward"]}


ENTRIES = ("torch", "m3d_conv3d_pack_weights", "m3d_conv3d_forward", "m3d_conv3d_forward_dilated", "m3d_conv3d_zw_bound_of", "m3d_conv3d_zw_pack",
           "m3d_conv3d_zw_pack_dgrad", "m3d_conv3d_zw_forward", "m3d_conv3d_zn_pack", "m3d_conv3d_zn_pack_dgrad", "m3d_conv3d_zn_forward",
           "m3d_conv3d_stem5_prepare_dgrad_weights", "m3d_conv3d_stem5_dgrad", "m3d_conv3d_gy_reduce", "m3d_conv3d_bias_grad",
           "m3d_conv3d_wgrad", "m3d_conv3d_wgrad_f16x2", "m3d_conv3d_wgrad_narrow", "m3d_conv3d_wgrad_dilated")


def test_fixture_covers_the_grid_and_every_entry_point(fixture):
    assert sorted(fixture) == sorted(case_key(*c) for c in cases())
    assert len(fixture) == len(LAYERS) * len(NEEDS) * len(SETTINGS) + len(FLIP_LAYERS) * len(SETTINGS)
    seen = set(itertools.chain.from_iterable(entry_names(r) for r in fixture.values()))
    assert seen == set(ENTRIES), seen ^ set(ENTRIES)


def test_launches_match_the_record(recorded, fixture):
    """the same entry points with the same arguments in the same order, forward and backward, on every grid point"""
    for key, want in fixture.items():
        got = recorded[key]
        assert got["forward"] == want["forward"], key
        assert got.get("backward") == want.get("backward"), key


def test_no_more_library_queries_per_call(recorded, fixture):
    for key, want in fixture.items():
        if "queries" in want:
            assert recorded[key]["queries"] <= want["queries"], (key, recorded[key]["queries"], want["queries"])


def test_switches_are_left_at_their_defaults(recorded):
    from m3d import compat
    assert (compat.get_conv_train(), compat.get_conv_train_narrow(), compat.get_conv_wgrad(), compat.get_conv_wgrad_narrow(),
            compat.get_conv_dilated()) == ("fp32", False, "fp32", False, "torch")


# ----------------------------------------------------------------------------- the plan itself
def routed(layer, dil):
    """the dilation conv3d() routes this layer's call under: 1, 2 or None (torch)"""
    _, _, dilation, padding, _ = LAYERS[layer]
    if layer.startswith("pad0") or dilation == 3:
        return None
    return 1 if dilation == 1 else (2 if dil == "m3d" else None)


def plans():
    """(layer, needs, setting, TrainSetting, plan) over the grid's library calls"""
    import __graft_entry__ as g
    g.build()
    from m3d import conv_plan as cp
    for layer, needs, setting in itertools.product(LAYERS, NEEDS, SETTINGS):
        dilation = routed(layer, setting[4])
        if dilation is None:
            continue
        xshape, (cout, cin, k), _, _, _ = LAYERS[layer]
        gx, gw, gb = NEEDS[needs]
        s = train_setting(cp, setting)
        yield layer, needs, setting, s, cp.plan_train_conv(s, xshape, (cout, cin, k, k, k), dilation, (gx, gw, bool(gb)))


def test_plan_is_a_pure_function_of_its_arguments():
    import __graft_entry__ as g
    g.build()
    from m3d import conv_plan as cp
    for fn in (cp.plan_train_conv, cp.plan_train_forward, cp.plan_train_backward, cp._train_rule):
        src = inspect.getsource(fn)
        assert "environ" not in src and "global" not in src, fn.__name__
    s = cp.TrainSetting(train="f16x2", min_units=0, narrow=0, wgrad="f16x2", wgrad_narrow=True, dilated="m3d")
    args = (s, (2, 64, 17, 33, 63), (64, 64, 3, 3, 3), 1, (True, True, True))
    assert len({cp.plan_train_conv(*args) for _ in range(3)}) == 1
    assert cp.TrainSetting()._asdict() == dict(train="fp32", min_units=None, narrow=None, wgrad="fp32", wgrad_narrow=False, dilated="torch",
                                               wgrad_narrow_f16=None, dilated_f16=None, wgrad_dilated_f16=None)
    with pytest.raises(AttributeError):
        s.train = "fp32"                                                    # immutable


def test_every_plan_field_takes_each_of_its_values_on_the_grid():
    from m3d import conv_plan as cp
    seen = {}
    for _, _, _, _, p in plans():
        for name, value in p._asdict().items():
            seen.setdefault(name, set()).add(value)
    assert seen == {"forward": {cp.TRAIN_FP32, cp.TRAIN_F16X2, cp.TRAIN_F16X2_NARROW, cp.TRAIN_DILATED},
                    "sweep": {False, True},
                    "dgrad": {None, cp.DGRAD_STEM, cp.TRAIN_FP32, cp.TRAIN_F16X2, cp.TRAIN_F16X2_NARROW, cp.TRAIN_DILATED},
                    "wgrad": {None, cp.WGRAD_FP32, cp.WGRAD_F16X2, cp.WGRAD_NARROW, cp.WGRAD_DILATED},
                    "gy_reduce": {False, True},
                    "gb": {None, cp.GB_REDUCE, cp.GB_BIAS_GRAD}}


def test_plan_agrees_with_the_rules_on_every_grid_point():
    """the kernel fields are train_conv_kernel / wgrad_kernel's rows; the rest follows from them as DESIGN's table says"""
    from m3d import conv_plan as cp
    for layer, needs, setting, s, p in plans():
        (B, _, D, H, W), (cout, cin, k), dilation, _, _ = LAYERS[layer]
        gx, gw, gb = NEEDS[needs]
        key = case_key(layer, needs, setting)
        if dilation == 2:
            assert p == cp.TrainConvPlan(cp.TRAIN_DILATED, False, cp.TRAIN_DILATED if gx else None, cp.WGRAD_DILATED if gw else None, False,
                                         cp.GB_BIAS_GRAD if gb else None), key
            continue
        kw = dict(min_units=cp.ZW_MIN_UNITS if s.min_units is None else s.min_units, k=k)
        if s.narrow is not None:
            kw.update(narrow=True, narrow_min_units=s.narrow)
        fwd = cp.train_conv_kernel("forward", B, cin, cout, D, H, W, s.train, **kw)
        dgrad = cp.train_conv_kernel("dgrad", B, cin, cout, D, H, W, s.train, **kw)
        wgrad = cp.wgrad_kernel(B, cin, cout, D, H, W, s.wgrad, k=k, narrow=s.wgrad_narrow)
        assert p.forward == fwd and p.sweep == (fwd != cp.TRAIN_FP32), key
        assert p.dgrad == (None if not gx else cp.DGRAD_STEM if k == 5 else dgrad), key
        assert p.wgrad == (wgrad if gw else None), key
        f16 = s.train == cp.TRAIN_F16X2
        f16_user = p.dgrad == cp.TRAIN_F16X2 or p.wgrad == cp.WGRAD_F16X2 or bool(gb)
        assert p.gy_reduce == ((f16 and f16_user) or p.dgrad == cp.TRAIN_F16X2_NARROW), key
        assert p.gb == (None if not gb else cp.GB_REDUCE if p.gy_reduce else cp.GB_BIAS_GRAD), key


def test_backward_has_no_routing_left():
    """no branch of _Conv3dFn.backward tests a switch or a mode string: it runs the plan's fields, the kernel kinds from two tables"""
    from m3d import compat, conv_plan as cp
    branches = [line.strip() for line in inspect.getsource(compat._Conv3dFn.backward).splitlines() if line.strip().startswith(("if ", "elif "))]
    assert len(branches) == 2
    for line in branches:                                                   # each tests one field of the plan against one kind
        assert re.fullmatch(r"(if|elif) (gy_reduce|(dgrad|wgrad|gb_from) == conv_plan\.[A-Z0-9_]+):", line), line
    assert not hasattr(compat, "_Conv3dDilated2Fn")
    for fn in (compat._Conv3dFn.forward, compat._Conv3dFn.backward):
        lines = [line for line in inspect.getsource(fn).splitlines() if "BACKWARD_FIELDS" not in line]
        assert not any("assert" in line or "_setting." in line for line in lines), fn.__name__
    assert len([line for line in inspect.getsource(compat._Conv3dFn.backward).splitlines() if "BACKWARD_FIELDS" in line]) == 1
    assert "BACKWARD_FIELDS" not in inspect.getsource(compat._Conv3dFn.forward)
    assert set(compat._CONV_KINDS) == {cp.TRAIN_FP32, cp.TRAIN_F16X2, cp.TRAIN_F16X2_NARROW, cp.TRAIN_DILATED, cp.TRAIN_DILATED_F16X2,
                                       cp.DGRAD_STEM}
    assert set(compat._WGRAD_KINDS) == {cp.WGRAD_FP32, cp.WGRAD_F16X2, cp.WGRAD_NARROW, cp.WGRAD_NARROW_F16X2, cp.WGRAD_DILATED,
                                        cp.WGRAD_DILATED_F16X2}
    assert len(compat._CONV_KINDS) == len(compat._WGRAD_KINDS) == 6         # (kinds of the two families share strings: no key collapsed)


# ----------------------------------------------------------------------------- when each field of the setting is read
DIL2_ROI = ((4, 32, 7, 7, 7), (32, 32, 3), 2, 2, True)          # the mask head's 7^3 RoI grid at dilation 2: both dilated f16x2 kernels take it
# field: (layer, base setting A as TrainSetting fields, value v): the smallest layer at which the field moves a launch; thresholds 0
FIELD_CASES = {
    "train": (LAYERS["body 64-64"], {}, "f16x2"),
    "min_units": (LAYERS["body 64-64"], dict(train="f16x2", min_units=1 << 30), 0),
    "narrow": (LAYERS["roi R16 256-256"], {}, 0),
    "wgrad": (LAYERS["work 2^27 128-256"], {}, "f16x2"),
    "wgrad_narrow": (LAYERS["roi R4 32-64"], {}, True),
    "wgrad_narrow_f16": (LAYERS["roi R4 32-64"], {}, 0),
    "dilated": (LAYERS["dil2 32-32"], dict(dilated="m3d"), "torch"),        # the backward of a library forward stays in the library
    "dilated_f16": (DIL2_ROI, dict(dilated="m3d"), 0),
    "wgrad_dilated_f16": (DIL2_ROI, dict(dilated="m3d"), 0),
}


def apply_train_setting(compat, s):
    """a whole TrainSetting through the eight setters"""
    compat.set_conv_train(s.train, s.min_units)
    compat.set_conv_train_narrow(s.narrow is not None, s.narrow)
    compat.set_conv_wgrad(s.wgrad)
    compat.set_conv_wgrad_narrow(s.wgrad_narrow)
    compat.set_conv_dilated(s.dilated)
    compat.set_conv_wgrad_narrow_f16(s.wgrad_narrow_f16 is not None, s.wgrad_narrow_f16)
    compat.set_conv_dilated_f16(s.dilated_f16 is not None, s.dilated_f16)
    compat.set_conv_wgrad_dilated_f16(s.wgrad_dilated_f16 is not None, s.wgrad_dilated_f16)
    assert compat._setting == s


def run_fields(compat, rec, layer, at_forward, at_backward):
    """-> {"forward": launches | "torch", "backward": launches}: the forward under the TrainSetting at_forward, the backward under at_backward"""
    xshape, (cout, cin, k), dilation, padding, contiguous = layer
    apply_train_setting(compat, at_forward)
    x, w, b = meta(xshape, True, contiguous), meta((cout, cin, k, k, k), True), meta((cout,), True)
    rec.take()
    y = compat.conv3d(x, w, b, 1, padding, dilation, 1)
    fwd, _ = rec.take()
    if isinstance(y, str):                                      # the stand-in for torch's conv3d
        return {"forward": "torch"}
    apply_train_setting(compat, at_backward)
    grads = torch.autograd.grad(y, [x, w, b], torch.empty(y.shape, device="meta").as_subclass(CudaMeta))
    assert all(g is not None for g in grads)
    return {"forward": fwd, "backward": rec.take()[0]}


def test_each_field_is_read_when_its_table_says():
    """one field at a time, in the form of the flip records: the forward under a base setting A, the field set to v before the backward.
    A FORWARD_FIELDS field: the call launches what it launches under A throughout; a BACKWARD_FIELDS field: its backward is the
    backward under "A with the field at v" throughout.  Each (A, v) moves a launch, so no field is tested vacuously."""
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        from m3d import compat, conv_plan as cp
        mp.setattr(compat, "_orig_conv3d", lambda *a: "torch")
        assert sorted(cp.FORWARD_FIELDS + cp.BACKWARD_FIELDS) == sorted(cp.TrainSetting._fields)
        assert set(cp.FORWARD_FIELDS) == {"train", "min_units", "narrow", "dilated", "dilated_f16"}
        assert set(cp.BACKWARD_FIELDS) == {"wgrad", "wgrad_narrow", "wgrad_narrow_f16", "wgrad_dilated_f16"}
        assert sorted(FIELD_CASES) == sorted(cp.TrainSetting._fields)
        try:
            for field, (layer, base, v) in FIELD_CASES.items():
                A = cp.TrainSetting(**base)
                Av = A._replace(**{field: v})
                under_a, under_v = run_fields(compat, rec, layer, A, A), run_fields(compat, rec, layer, Av, Av)
                assert under_a != under_v and under_a["forward"] != "torch", field
                got = run_fields(compat, rec, layer, A, Av)
                if field in cp.FORWARD_FIELDS:
                    assert got == under_a, field
                else:
                    assert got["forward"] == under_a["forward"] == under_v["forward"], field
                    assert got["backward"] == under_v["backward"] != under_a["backward"], field
        finally:
            apply_train_setting(compat, cp.TrainSetting())
