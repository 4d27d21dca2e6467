"""CPU: what a training conv launches with m3d.compat.set_conv_dilated_f16, on meta tensors against the recording double of the library
(tests/conv_record.py).

With the switch off, the records over the whole grid of tests/test_conv_train_dispatch.py, flips included, are the ones
tests/golden/conv_train_dispatch.json.gz holds, with no library query more.

The grid's own dilation-2 layers ("dil2 32-32") are 14 wide: the dilation-2 f16x2 kernel takes maps at most 8 wide
(m3d_conv3d_zn_dilated_supported), so with the switch on they launch what they launched - that is pinned here too.  The layers that
move are the mask head's on the 7^3 RoI grid, added below under "dil2 roi ...": with the switch on under dil=m3d their forward and
backward-data run on m3d_conv3d_zn_dilated_forward (dilation argument 2, a swept bound in front of the forward, m3d_conv3d_gy_reduce
in front of the dgrad, which then also gives the bias gradient), the weight gradient stays on m3d_conv3d_wgrad_dilated with the
arguments it had, and nothing else moves; a direction whose launched input channels are no multiple of 16 stays on the fp32 kernel.
Under dil=torch nothing moves.  The flip records show that the switch is read at forward time.  plan_train_conv under a setting with
dilated_f16 agrees with the table of its docstring on every grid point, and with None it is the plan of the setting without it."""
import gzip
import itertools
import json

import pytest
import torch

import test_conv_train_dispatch as G
from conv_record import CudaMeta, install

# name: (x shape, (cout, cin, k), dilation, padding, contiguous x): the 7^3 RoI grid at dilation 2
ROI_LAYERS = {
    "dil2 roi R4 32-32": ((4, 32, 7, 7, 7), (32, 32, 3), 2, 2, True),            # 8 units: below any threshold but 0
    "dil2 roi R300 32-32": ((300, 32, 7, 7, 7), (32, 32, 3), 2, 2, True),        # 600 units
    "dil2 roi R4 24-32": ((4, 32, 7, 7, 7), (24, 32, 3), 2, 2, True),            # cout 24: the dgrad's launched cin is no multiple of 16
    "dil2 roi R4 32-24": ((4, 24, 7, 7, 7), (32, 24, 3), 2, 2, True),            # cin 24: the forward's is not
    "dil2 roi R4 32-32 strided": ((4, 32, 7, 7, 7), (32, 32, 3), 2, 2, False),   # not contiguous: torch, whatever the switches say
}
LAYERS = dict(G.LAYERS, **ROI_LAYERS)
OFF, ON0, ON = (False, None), (True, 0), (True, None)          # set_conv_dilated_f16(on, min_units)
NEW, REDUCE, SWEEP = "m3d_conv3d_zn_dilated_forward", "m3d_conv3d_gy_reduce", "m3d_conv3d_zw_bound_of"
OLD, WGRAD, BIAS = "m3d_conv3d_forward_dilated", "m3d_conv3d_wgrad_dilated", "m3d_conv3d_bias_grad"


def run_case(compat, rec, layer, needs, setting, df, df_backward=None):
    """-> {"forward": launches | "torch", "backward": launches, "queries": n}; df_backward: every OLD switch turned over and the new one
    set to this between the forward and the backward (None: all left alone)"""
    xshape, (cout, cin, k), dilation, padding, contiguous = LAYERS[layer]
    gx, gw, gb = G.NEEDS[needs]
    G.apply_setting(compat, setting)
    compat.set_conv_dilated_f16(*df)
    x, w = G.meta(xshape, gx, contiguous), G.meta((cout, cin, k, k, k), gw)
    b = None if gb is None else G.meta((cout,), gb)
    rec.take()
    y = compat.conv3d(x, w, b, 1, padding, dilation, 1)
    fwd, queries = rec.take()
    if isinstance(y, str):                                      # the stand-in for torch's conv3d
        assert not fwd
        return {"forward": "torch"}
    if df_backward is not None:
        G.apply_setting(compat, G.flipped(setting))
        compat.set_conv_dilated_f16(*df_backward)
    gy = torch.empty(y.shape, device="meta").as_subclass(CudaMeta)
    grads = torch.autograd.grad(y, [t for t in (x, w, b) if t is not None and t.requires_grad], gy)
    assert all(g is not None for g in grads)
    bwd, q2 = rec.take()
    return {"forward": fwd, "backward": bwd, "queries": queries + q2}


def dilated(layer):
    return LAYERS[layer][2] == 2


@pytest.fixture(scope="module")
def recorded():
    """{"layer | needs | setting | tag": record}; tag off over every layer, on0 / on / flip_on / flip_off over the dilation-2 layers"""
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        from m3d import compat
        mp.setattr(compat, "_orig_conv3d", lambda *a: "torch")
        out = {}
        try:
            for layer, needs, setting in itertools.product(LAYERS, G.NEEDS, G.SETTINGS):
                key = (layer, needs, G.setting_key(setting))
                out[key + ("off",)] = run_case(compat, rec, layer, needs, setting, OFF)
                if dilated(layer):
                    out[key + ("on0",)] = run_case(compat, rec, layer, needs, setting, ON0)
                    out[key + ("on",)] = run_case(compat, rec, layer, needs, setting, ON)
            for layer, setting in itertools.product(LAYERS, G.SETTINGS):
                key = (layer, "xwb", G.setting_key(setting))
                if layer in G.FLIP_LAYERS:
                    out[key + ("flip",)] = run_case(compat, rec, layer, "xwb", setting, OFF, df_backward=OFF)
                if dilated(layer):
                    out[key + ("flip_on",)] = run_case(compat, rec, layer, "xwb", setting, OFF, df_backward=ON0)
                    out[key + ("flip_off",)] = run_case(compat, rec, layer, "xwb", setting, ON0, df_backward=OFF)
        finally:
            G.apply_setting(compat, G.DEFAULT)
            compat.set_conv_dilated_f16(False)
        return json.loads(json.dumps({" | ".join(k): v for k, v in out.items()}))


def get(recorded, layer, needs, setting, tag):
    return recorded[" | ".join((layer, needs, G.setting_key(setting), tag))]


def same(a, b):
    return a["forward"] == b["forward"] and a.get("backward") == b.get("backward")


def names(launches):
    return [launch[0] for launch in launches]


# ----------------------------------------------------------------------------- off: the golden record
def test_switch_off_is_the_golden_record(recorded):
    with gzip.open(G.FIXTURE, "rt") as f:
        fixture = json.load(f)
    seen = 0
    for layer, needs, setting, flip in G.cases():
        want = fixture[G.case_key(layer, needs, setting, flip)]
        got = get(recorded, layer, needs, setting, "flip" if flip else "off")
        assert same(got, want), (layer, needs, setting, flip)
        if "queries" in want:
            assert got["queries"] <= want["queries"], (layer, needs, setting, flip)      # no additional library query with the switch off
        seen += 1
    assert seen == len(fixture)
    for record in recorded.values():
        if not record["forward"] == "torch" and NEW in names(record["forward"] + record["backward"]):
            break
    else:
        raise AssertionError("no record launches " + NEW)


# ----------------------------------------------------------------------------- on
def takes(cp, ci, co, xshape, min_units):
    B, _, D, H, W = xshape
    L = cp.ops.lib()
    return bool(L.m3d_conv3d_zn_dilated_supported(ci, co, D, H, W, 2)) and L.m3d_conv3d_zn_dilated_launch_units(B, ci, co, D, H, W, 2) >= min_units


def expected(cp, layer, needs, off, min_units):
    """the record with the switch on at `min_units`, from the record with it off and the rules of the issue"""
    xshape, (cout, cin, k), _, _, _ = LAYERS[layer]
    B, _, D, H, W = xshape
    gx, gw, gb = (bool(v) for v in G.NEEDS[needs])
    fwd_new, dgrad_new = takes(cp, cin, cout, xshape, min_units), gx and takes(cp, cout, cin, xshape, min_units)
    forward = off["forward"]
    if fwd_new:
        assert names(forward) == ["m3d_conv3d_pack_weights", OLD]
        old = forward[-1]
        assert old[4:10] == [B, cin, cout, D, H, W] and old[10:12] == [3, 2]          # k, dilation
        shift = "ptr" if G.NEEDS[needs][2] is not None else "null"
        forward = [[SWEEP, "ptr", B * cin * D * H * W, "ptr", "null"],
                   ["m3d_conv3d_zn_pack", "ptr", cin, cout, "ptr", "null"],
                   [NEW, "ptr", "ptr", "ptr", B, cin, cout, D, H, W, 2, "null", shift, 0, "ptr", "null", "null"]]
    backward = list(off["backward"])
    if dgrad_new:
        at = [i for i, launch in enumerate(backward) if launch[0] == OLD]
        assert len(at) == 1 and backward[at[0] - 1][0] == "m3d_conv3d_pack_weights" and at[0] == 1
        # conv3d_gy_reduce: the workspace-size call, then the pass (gb only where the bias gradient is needed)
        backward[0:2] = [[REDUCE, "null", B, cout, D, H, W, "null", "null", "null", "ref", "null"],
                         [REDUCE, "ptr", B, cout, D, H, W, "ptr" if gb else "null", "ptr", "ptr", "ref", "null"],
                         ["m3d_conv3d_zn_pack_dgrad", "ptr", cin, cout, "ptr", "null"],
                         [NEW, "ptr", "ptr", "ptr", B, cout, cin, D, H, W, 2, "null", "null", 0, "ptr", "null", "null"]]
        if gb:                                             # the reduce gives the bias gradient: no m3d_conv3d_bias_grad
            assert backward[-1][0] == BIAS
            backward.pop()
    return {"forward": forward, "backward": backward}


def test_on_under_m3d_moves_forward_and_dgrad_of_the_narrow_dilated_layers_and_nothing_else(recorded):
    from m3d import conv_plan as cp
    moved = {"forward": 0, "dgrad": 0, "one direction": 0}
    for layer, needs, setting in itertools.product(LAYERS, G.NEEDS, G.SETTINGS):
        if not dilated(layer):
            continue
        key = (layer, needs, setting)
        off = get(recorded, layer, needs, setting, "off")
        for tag, min_units in (("on0", 0), ("on", cp.ZN_DILATED_MIN_UNITS)):
            on = get(recorded, layer, needs, setting, tag)
            if setting[4] == "torch" or off["forward"] == "torch":
                assert same(on, off) and on["forward"] == "torch", key          # under dil=torch nothing moves
                continue
            if layer not in ROI_LAYERS:
                assert same(on, off), key                   # 14 (or 3 x dilation) wide: the kernel does not take them
                continue
            want = expected(cp, layer, needs, off, min_units)
            assert on["forward"] == want["forward"], (key, tag)
            assert on["backward"] == want["backward"], (key, tag)
            f, d = NEW in names(on["forward"]), NEW in names(on["backward"])
            assert (REDUCE in names(on["backward"])) == d and (BIAS in names(on["backward"])) == (bool(G.NEEDS[needs][2]) and not d), key
            if G.NEEDS[needs][1]:                           # gw: the same launch as with the switch off
                assert [l for l in on["backward"] if l[0] == WGRAD] == [l for l in off["backward"] if l[0] == WGRAD] != [], key
            moved["forward"] += f
            moved["dgrad"] += d
            moved["one direction"] += f != d and bool(G.NEEDS[needs][0])
    assert all(moved.values()), moved
    # the default threshold: the 8-unit layers stay, the 600-unit layer moves
    s = next(s for s in G.SETTINGS if s[4] == "m3d")
    assert same(get(recorded, "dil2 roi R4 32-32", "xwb", s, "on"), get(recorded, "dil2 roi R4 32-32", "xwb", s, "off"))
    assert 8 < cp.ZN_DILATED_MIN_UNITS <= 600
    assert NEW in names(get(recorded, "dil2 roi R300 32-32", "xwb", s, "on")["forward"])


def test_the_switch_is_read_at_forward_time(recorded):
    """flip_on: off at the forward, on (and every older switch turned over) before the backward - the backward of a library forward is
    the off record's, except for what the two wgrad switches, read at backward time, say; flip_off the other way round"""
    for layer, setting in itertools.product(LAYERS, G.SETTINGS):
        if not dilated(layer):
            continue
        off, on = get(recorded, layer, "xwb", setting, "off"), get(recorded, layer, "xwb", setting, "on0")
        flip_on, flip_off = get(recorded, layer, "xwb", setting, "flip_on"), get(recorded, layer, "xwb", setting, "flip_off")
        # (the weight gradient of a dilation-2 layer is m3d_conv3d_wgrad_dilated under every wgrad switch: the whole record is comparable)
        assert same(flip_on, off), (layer, setting)
        assert same(flip_off, on), (layer, setting)


def test_switches_are_left_at_their_defaults(recorded):
    from m3d import compat
    assert (compat.get_conv_train(), compat.get_conv_train_narrow(), compat.get_conv_wgrad(), compat.get_conv_wgrad_narrow(),
            compat.get_conv_dilated(), compat.get_conv_wgrad_narrow_f16(), compat.get_conv_dilated_f16()) == \
        ("fp32", False, "fp32", False, "torch", False, False)


# ----------------------------------------------------------------------------- the plan
def test_the_plan_agrees_with_the_table_on_every_grid_point():
    import __graft_entry__ as g
    g.build()
    from m3d import conv_plan as cp
    assert cp.TRAIN_DILATED_F16X2 == "f16x2 dilated"
    new = 0
    for layer, needs, setting in itertools.product(LAYERS, G.NEEDS, G.SETTINGS):
        xshape, (cout, cin, k), dilation, padding, _ = LAYERS[layer]
        if layer.startswith("pad0") or dilation == 3:
            continue
        routed = 1 if dilation == 1 else (2 if setting[4] == "m3d" else None)
        if routed is None:
            continue
        s = G.train_setting(cp, setting)
        gx, gw, gb = (bool(v) for v in G.NEEDS[needs])
        args = (s, xshape, (cout, cin, k, k, k), routed, (gx, gw, gb))
        base = cp.plan_train_conv(*args)
        assert cp.plan_train_conv(s._replace(dilated_f16=None), *args[1:]) == base  # None: today's plan
        assert cp.plan_train_forward(*args[:4]) == cp.plan_train_forward(s._replace(dilated_f16=None), *args[1:4]) == tuple(base[:2])
        for min_units in (0, cp.ZN_DILATED_MIN_UNITS, 1 << 40):
            on = s._replace(dilated_f16=min_units)
            p = cp.plan_train_conv(on, *args[1:])
            assert cp.plan_train_forward(on, *args[1:4]) == tuple(p[:2])
            assert cp.plan_train_backward(on, *args[1:]) == tuple(p[2:])
            if routed == 1:
                assert p == base, (layer, needs, setting)
                continue
            f = takes(cp, cin, cout, xshape, min_units)
            d = gx and takes(cp, cout, cin, xshape, min_units)
            want = cp.TrainConvPlan(forward=cp.TRAIN_DILATED_F16X2 if f else cp.TRAIN_DILATED, sweep=f,
                                    dgrad=None if not gx else cp.TRAIN_DILATED_F16X2 if d else cp.TRAIN_DILATED,
                                    wgrad=cp.WGRAD_DILATED if gw else None, gy_reduce=d,
                                    gb=None if not gb else cp.GB_REDUCE if d else cp.GB_BIAS_GRAD)
            assert p == want, (layer, needs, setting, min_units)
            new += f or d
        # without set_conv_dilated("m3d") in the setting the switch has no effect on the plan either
        if dilation == 2:
            assert cp.plan_train_conv(s._replace(dilated="torch", dilated_f16=0), *args[1:]) == base == \
                cp.plan_train_conv(s._replace(dilated="torch"), *args[1:])
    assert new > 0
