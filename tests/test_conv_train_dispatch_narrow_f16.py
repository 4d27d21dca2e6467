"""CPU: what a training conv launches with m3d.compat.set_conv_wgrad_narrow_f16, on meta tensors against the recording double of the
library (tests/conv_record.py), over the layers of tests/test_conv_train_dispatch.py at which the new route can change, crossed with
every combination of the five older switches.

With the switch on and min_work = 0 the record of a call equals the record with the switch off, except that the weight-gradient launch
of every layer the kernel takes (k = 3, dilation 1, W <= 8, cin and cout multiples of 32) is m3d_conv3d_wgrad_narrow_f16x2, with both
bound pointers non-null and a bound sweep in front of it for each bound the plan did not already hold.  With the default threshold the
layers below it are unchanged.  The "flip" records pin that the switch is read when the backward runs.  The switch-off records are the
ones tests/golden/conv_train_dispatch.json.gz holds."""
import gzip
import itertools
import json
import os

import pytest
import torch

from conv_record import DEFAULT, NEEDS, SETTINGS, CudaMeta, install, meta, setting_key, train_setting

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_train_dispatch.json.gz")

# name: (x shape, (cout, cin, k), dilation, padding): the shapes of tests/test_conv_train_dispatch.py::LAYERS under these names
LAYERS = {
    "roi R4 32-64": ((4, 32, 7, 7, 7), (64, 32, 3), 1, 1),
    "roi R16 256-256": ((16, 256, 7, 7, 7), (256, 256, 3), 1, 1),
    "roi R15 256-256": ((15, 256, 7, 7, 7), (256, 256, 3), 1, 1),
    "roi R70 256-32": ((70, 256, 7, 7, 7), (32, 256, 3), 1, 1),
    "map W8 64-64": ((2, 64, 9, 10, 8), (64, 64, 3), 1, 1),
    "map W12 64-64": ((2, 64, 9, 10, 12), (64, 64, 3), 1, 1),
    "body 64-64": ((2, 64, 17, 33, 63), (64, 64, 3), 1, 1),
    "dil2 32-32": ((4, 32, 14, 14, 14), (32, 32, 3), 2, 2),
    "k1 64-35": ((2, 64, 17, 33, 63), (35, 64, 1), 1, 0),
}
TAKEN = ("roi R4 32-64", "roi R16 256-256", "roi R15 256-256", "roi R70 256-32", "map W8 64-64")     # W <= 8, channels multiples of 32, k = 3

OFF, ON0, ON = (False, None), (True, 0), (True, None)            # set_conv_wgrad_narrow_f16(on, min_work)

OLD_WGRADS = ("m3d_conv3d_wgrad", "m3d_conv3d_wgrad_f16x2", "m3d_conv3d_wgrad_narrow")
NEW = "m3d_conv3d_wgrad_narrow_f16x2"
SWEEP = "m3d_conv3d_zw_bound_of"


def apply_setting(compat, setting, nf):
    train, narrow, wgrad, wn, dil = setting
    compat.set_conv_train(*train)
    compat.set_conv_train_narrow(*narrow)
    compat.set_conv_wgrad(wgrad)
    compat.set_conv_wgrad_narrow(wn)
    compat.set_conv_dilated(dil)
    compat.set_conv_wgrad_narrow_f16(*nf)


def run_case(compat, rec, layer, needs, setting, nf, nf_backward=None):
    """-> {"forward": launches | "torch", "backward": launches, "queries": n}; nf_backward: the new switch as set between the forward
    and the backward (None: left alone)"""
    xshape, (cout, cin, k), dilation, padding = LAYERS[layer]
    gx, gw, gb = NEEDS[needs]
    apply_setting(compat, setting, nf)
    x, w = meta(xshape, gx), meta((cout, cin, k, k, k), gw)
    b = None if gb is None else meta((cout,), gb)
    rec.take()
    y = compat.conv3d(x, w, b, 1, padding, dilation, 1)
    fwd, queries = rec.take()
    if isinstance(y, str):                                      # the stand-in for torch's conv3d
        assert not fwd
        return {"forward": "torch"}
    if nf_backward is not None:
        compat.set_conv_wgrad_narrow_f16(*nf_backward)
    gy = torch.empty(y.shape, device="meta").as_subclass(CudaMeta)
    grads = torch.autograd.grad(y, [t for t in (x, w, b) if t is not None and t.requires_grad], gy)
    assert all(g is not None for g in grads)
    bwd, q2 = rec.take()
    return {"forward": fwd, "backward": bwd, "queries": queries + q2}


@pytest.fixture(scope="module")
def recorded():
    """{(layer, needs, setting key, tag): record}, tag in off / on0 / on / flip_on / flip_off"""
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        from m3d import compat
        mp.setattr(compat, "_orig_conv3d", lambda *a: "torch")
        out = {}
        try:
            for layer, needs, setting in itertools.product(LAYERS, NEEDS, SETTINGS):
                key = (layer, needs, setting_key(setting))
                out[key + ("off",)] = run_case(compat, rec, layer, needs, setting, OFF)
                out[key + ("on0",)] = run_case(compat, rec, layer, needs, setting, ON0)
                out[key + ("on",)] = run_case(compat, rec, layer, needs, setting, ON)
                if needs == "xwb":
                    out[key + ("flip_on",)] = run_case(compat, rec, layer, needs, setting, OFF, nf_backward=ON0)
                    out[key + ("flip_off",)] = run_case(compat, rec, layer, needs, setting, ON0, nf_backward=OFF)
        finally:
            apply_setting(compat, DEFAULT, OFF)
        return json.loads(json.dumps({" | ".join(k): v for k, v in out.items()}))


def get(recorded, layer, needs, setting, tag):
    return recorded[" | ".join((layer, needs, setting_key(setting), tag))]


def grid():
    return itertools.product(LAYERS, NEEDS, SETTINGS)


def wgrad_span(backward, names):
    """(a, b): backward[a:b] is the weight-gradient launch with the bound sweeps in front of it (the only sweeps a backward makes)"""
    at = [i for i, launch in enumerate(backward) if launch[0] in names]
    assert len(at) == 1, backward
    a = at[0]
    while a > 0 and backward[a - 1][0] == SWEEP:
        a -= 1
    return a, at[0] + 1


def test_switch_off_is_the_golden_record(recorded):
    with gzip.open(FIXTURE, "rt") as f:
        fixture = json.load(f)
    for layer, needs, setting in grid():
        want = fixture["%s | %s | %s" % (layer, needs, setting_key(setting))]
        got = get(recorded, layer, needs, setting, "off")
        assert got["forward"] == want["forward"] and got.get("backward") == want.get("backward"), (layer, needs, setting)
        if "queries" in want:
            assert got["queries"] <= want["queries"], (layer, needs, setting)          # no additional library query with the switch off


def test_min_work_0_moves_the_wgrad_launch_of_every_taken_layer_and_nothing_else(recorded):
    from m3d import conv_plan as cp
    moved = 0
    for layer, needs, setting in grid():
        off, on = get(recorded, layer, needs, setting, "off"), get(recorded, layer, needs, setting, "on0")
        key = (layer, needs, setting)
        assert on["forward"] == off["forward"], key
        gw = NEEDS[needs][1]
        if layer not in TAKEN or not gw or off["forward"] == "torch":
            assert on.get("backward") == off.get("backward"), key
            assert all(launch[0] != NEW for launch in on.get("backward", [])), key
            continue
        xshape, (cout, cin, k), dilation, _ = LAYERS[layer]
        assert all(launch[0] != NEW for launch in off["backward"]), key
        a, b = wgrad_span(off["backward"], OLD_WGRADS)
        c, d = wgrad_span(on["backward"], (NEW,))
        assert on["backward"][:c] == off["backward"][:a] and on["backward"][d:] == off["backward"][b:], key      # gy_reduce, dgrad, gb
        launch = on["backward"][d - 1]
        B, _, D, H, W = xshape
        assert launch[:4] == [NEW, "ptr", "ptr", "ptr"] and launch[4:10] == [B, cin, cout, D, H, W], key
        assert launch[10] == "ptr" and launch[11] == "ptr" and launch[12] == "ptr", key                          # x_max, gy_max, workspace
        assert launch[13] == cp.ops.conv3d_wgrad_narrow_f16x2_plan(B, cin, cout, D, H, W)["slots"] * 27 * cin * cout * 4, key
        # a sweep exactly for each bound the plan did not hold: x's from the forward's sweep, gy's from gy_reduce
        p = cp.plan_train_conv(train_setting(cp, setting)._replace(wgrad_narrow_f16=0), xshape, (cout, cin, k, k, k), dilation,
                               tuple(bool(v) for v in NEEDS[needs]))
        assert p.wgrad == cp.WGRAD_NARROW_F16X2, key
        assert d - 1 - c == (not p.sweep) + (not p.gy_reduce), key
        assert any(launch[0] == "m3d_conv3d_gy_reduce" for launch in on["backward"]) == p.gy_reduce, key
        moved += 1
    assert moved == len(TAKEN) * 3 * len(SETTINGS)


def test_the_default_threshold_leaves_the_layers_below_it_alone(recorded):
    from m3d import conv_plan as cp
    below = above = 0
    for layer, needs, setting in grid():
        (B, _, D, H, W), (cout, cin, _), _, _ = LAYERS[layer]
        routed = B * D * H * W * cin * cout >= cp.WGRAD_NARROW_F16X2_MIN_WORK
        want = get(recorded, layer, needs, setting, "on0" if routed else "off")
        got = get(recorded, layer, needs, setting, "on")
        assert got["forward"] == want["forward"] and got.get("backward") == want.get("backward"), (layer, needs, setting)
        if layer in TAKEN:
            below, above = below + (not routed), above + routed
    assert below > 0                                             # "roi R4 32-64": 2^18.4 products per tap


def test_the_switch_is_read_when_the_backward_runs(recorded):
    for layer, setting in itertools.product(LAYERS, SETTINGS):
        off, on = get(recorded, layer, "xwb", setting, "off"), get(recorded, layer, "xwb", setting, "on0")
        flip_on, flip_off = get(recorded, layer, "xwb", setting, "flip_on"), get(recorded, layer, "xwb", setting, "flip_off")
        assert flip_on["forward"] == on["forward"] and flip_on.get("backward") == on.get("backward"), (layer, setting)
        assert flip_off["forward"] == off["forward"] and flip_off.get("backward") == off.get("backward"), (layer, setting)


def test_switches_are_left_at_their_defaults(recorded):
    from m3d import compat
    assert (compat.get_conv_train(), compat.get_conv_train_narrow(), compat.get_conv_wgrad(), compat.get_conv_wgrad_narrow(),
            compat.get_conv_dilated(), compat.get_conv_wgrad_narrow_f16()) == ("fp32", False, "fp32", False, "torch", False)
