"""CPU: which library entry point runs each backbone / RPN convolution, pinned against a launch record.

The real entry points - DetectorM3D.conv_body + rpn (detection), DetectorM3D.conv_work (bench.py's roofline bookkeeping) and
PRMEngine.forward_response (PRM mode) - run on meta tensors against a recording double of the library: the pure host queries
(m3d_*_supported, _score, _bytes, ...) go through to the real libm3d.so, because the real decision code must run; every other entry
point is not called but written down (its name, every integer argument, null / non-null for every pointer argument).
tests/golden/conv_dispatch.json.gz holds what the commit before the planner (m3d/conv_plan.py) asked for
(tests/golden/gen_conv_dispatch.py writes it); the launches, the conv_work records and ZwConv3d.units() must not move.

A "pass" is one call on a detector that has seen the shape before (each pass runs twice; both must launch the same): the number of
library queries it makes is what a step of a running pipeline pays, and it may not exceed the recorded one.
"""
import ctypes as C
import gzip
import itertools
import json
import os

import pytest
import torch

from conv_record import CudaMeta, install

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json.gz")

NETS = {"stride8": dict(stride=8, num_anchors=35), "stride4": dict(stride=4, num_anchors=14)}
BATCHES = (1, 4)
ENVS = ({}, {"M3D_WINO": "1"}, {"M3D_WINO": "0"}, {"M3D_CONV_F16": "0"})
SIZES = ((128, 128, 128), (64, 64, 64), (32, 96, 96), (16, 32, 32), (48, 40, 24), (24, 24, 24), (64, 64, 24))
HUGE = (512, 512, 512)          # conv2a's batch item is 2 GiB: batch 1, detection path and conv_work only
GUARD = 0x7FFFFFFF              # bytes of one batch item from which the Winograd / f16x2 kernels' 32-bit offsets no longer reach
ZW_LAYERS = ((32, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256))      # (cin, cout) of the 3^3 convs of both nets

# the 2-D Winograd plan table (tests/golden/wino2_plan.json.gz, written by tests/golden/gen_wino2_plan.py): every host query of
# conv3d_wino2.hip over batch x layer x depth x (height = width), and the bytes of the stem's rows pack
PLAN_FIXTURE = os.path.join(ROOT, "tests", "golden", "wino2_plan.json.gz")
PLAN_LAYERS = ZW_LAYERS + ((4, 8), (64, 35))
PLAN_DEPTHS = (4, 9, 16, 64)
PLAN_WIDTHS = (8, 11, 12, 23, 24, 40, 47, 48, 64, 70, 128)
STEM_COUTS = (8, 32, 35, 40, 64, 128, 256)
M3D_EUNSUPPORTED = -4

DETECTION_ENTRIES = ("m3d_conv3d_forward", "m3d_conv3d_forward_pool2", "m3d_conv3d_wino_forward", "m3d_conv3d_wino_forward_pool2",
                     "m3d_conv3d_wino2_forward_ws", "m3d_conv3d_wino2_forward_pool2", "m3d_conv3d_zw_forward pool=0",
                     "m3d_conv3d_zw_forward pool=1", "m3d_conv3d_stem_wino_forward_bound", "m3d_maxpool3d_2x_forward",
                     "m3d_conv3d_zw_bound_of", "m3d_conv3d_forward_split_sigmoid")
# PRM mode needs the pool's arg-max (only the direct and the 2-D Winograd pool kernels give it), keeps pooled layers off f16x2 and
# un-fused Winograd, and has no F(2,5) stem launch
PRM_ENTRIES = ("m3d_conv3d_forward", "m3d_conv3d_forward_pool2", "m3d_conv3d_wino_forward", "m3d_conv3d_wino2_forward_ws",
               "m3d_conv3d_wino2_forward_pool2_argmax", "m3d_conv3d_zw_forward pool=0", "m3d_maxpool3d_2x_forward",
               "m3d_conv3d_zw_bound_of", "m3d_conv3d_forward_split_sigmoid")


def params(net):
    from m3d.synth import make_params
    return {k: v.to("meta").as_subclass(CudaMeta) for k, v in make_params(mlp_dim=64, **NETS[net]).items()}


def config(net):
    from m3d.config import Cfg
    return Cfg.nuclei() if net == "stride8" else Cfg.soma()


def env_key(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items())) or "default"


def case_key(net, batch, size, env):
    return "%s b%d %dx%dx%d %s" % ((net, batch) + tuple(size) + (env_key(env),))


def cases():
    for net, env in itertools.product(NETS, ENVS):
        for batch, size in itertools.product(BATCHES, SIZES):
            yield net, batch, size, env
        yield net, 1, HUGE, env


def set_env(mp, env):
    for k in ("M3D_WINO", "M3D_CONV_F16"):
        mp.delenv(k, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)


def twice(rec, fn):
    """one pass = fn() on a detector that has seen the shape: (launches, queries) of the second of two calls, which must launch alike"""
    fn()
    first, _ = rec.take()
    fn()
    second, queries = rec.take()
    assert first == second
    return second, queries


def record_case(rec, det, prm, batch, size):
    """what one case asks of the library; prm = None leaves the PRM forward out (batch items of 2 GiB and more)"""
    x = torch.empty((batch, 1) + tuple(size), device="meta")
    rec.take()
    out = {}
    out["detection"], out["detection_queries"] = twice(rec, lambda: det.rpn(det.conv_body(x)))
    out["conv_work"] = det.conv_work(batch, tuple(size))
    out["conv_work_queries"] = rec.take()[1]
    if prm is not None:
        out["prm_forward"], out["prm_forward_queries"] = twice(rec, lambda: prm.forward_response(x))
    return out


def record_all(mp):
    """the whole grid: {"construct": {net env: launches of DetectorM3D() + PRMEngine()}, "cases": {key: record_case}, "zw_units": [...]}"""
    rec = install(mp)
    from m3d.model import DetectorM3D
    from m3d.prm import PRMEngine
    from m3d import ops
    out = {"construct": {}, "cases": {}, "zw_units": []}
    for net, env in itertools.product(NETS, ENVS):
        set_env(mp, env)
        rec.take()
        det = DetectorM3D(params(net), config(net))
        prm = PRMEngine(det)
        out["construct"]["%s %s" % (net, env_key(env))] = rec.take()[0]
        for n, batch, size, e in cases():
            if (n, e) == (net, env):
                out["cases"][case_key(net, batch, size, env)] = record_case(rec, det, None if size == HUGE else prm, batch, size)
    set_env(mp, {})
    shapes = set()
    for batch, size in itertools.product(BATCHES, SIZES):
        for s in range(4):
            shapes.add((batch,) + tuple(v >> s for v in size))
    for batch, (d, h), w in itertools.product(BATCHES, ((7, 9), (15, 21), (33, 5)), (12, 23, 24, 25, 33)):
        shapes.add((batch, d, h, w))
    for cin, cout in ZW_LAYERS:
        zw = ops.ZwConv3d(torch.empty((cout, cin, 3, 3, 3), device="meta"))
        for b, d, h, w in sorted(shapes):
            out["zw_units"].append([cin, cout, b, d, h, w, int(zw.units((b, cin, d, h, w)))])
    return json.loads(json.dumps(out))          # as the fixture reads back (tuples -> lists)


def entry_names(launches):
    for r in launches:
        ints = [a for a in r[1:] if isinstance(a, int)]
        yield r[0] + (" pool=%d" % ints[7] if r[0] == "m3d_conv3d_zw_forward" else "")


def item_bytes(launch):
    """bytes of one batch item of a conv launch's input: its first integer arguments are B, cin, cout, D, H, W"""
    _, cin, _, d, h, w = [a for a in launch[1:] if isinstance(a, int)][:6]
    return cin * d * h * w * 4


@pytest.fixture(scope="module")
def recorded():
    with pytest.MonkeyPatch.context() as mp:
        return record_all(mp)


@pytest.fixture(scope="module")
def fixture():
    with gzip.open(FIXTURE, "rt") as f:
        return json.load(f)


def test_fixture_covers_every_entry_point(fixture):
    assert sorted(fixture["cases"]) == sorted(case_key(*c) for c in cases())
    det = set(itertools.chain.from_iterable(entry_names(c["detection"]) for c in fixture["cases"].values()))
    prm = set(itertools.chain.from_iterable(entry_names(c.get("prm_forward", [])) for c in fixture["cases"].values()))
    assert not set(DETECTION_ENTRIES) - det, set(DETECTION_ENTRIES) - det
    assert not set(PRM_ENTRIES) - prm, set(PRM_ENTRIES) - prm
    for key, c in fixture["cases"].items():
        assert ("prm_forward" in c) == ("512x512x512" not in key), key


def test_construction_launches(recorded, fixture):
    """the same weight packs are made when a detector and its PRM engine are built (as a multiset: packs of different layers are
    independent launches, and which layer packs first is not behaviour)"""
    for key, want in fixture["construct"].items():
        assert sorted(recorded["construct"][key], key=json.dumps) == sorted(want, key=json.dumps), key


@pytest.mark.parametrize("what", ["detection", "prm_forward", "conv_work"])
def test_launches_and_conv_work_match_the_record(recorded, fixture, what):
    for key, want in fixture["cases"].items():
        if what in want:
            assert recorded["cases"][key][what] == want[what], (key, what)


def test_no_more_library_queries_per_pass(recorded, fixture):
    for key, want in fixture["cases"].items():
        for what in ("detection_queries", "conv_work_queries", "prm_forward_queries"):
            if what in want:
                assert recorded["cases"][key][what] <= want[what], (key, what, recorded["cases"][key][what], want[what])


def test_zw_units_match_the_record(recorded, fixture):
    assert recorded["zw_units"] == fixture["zw_units"]


def test_prm_forward_keeps_32bit_kernels_below_the_guard():
    """PRM mode on a 512^3 tile (conv2a's batch item is 2 GiB): no Winograd and no f16x2 launch on an item at or above the guard.
    (The commit the fixture was recorded at ran m3d_conv3d_wino2_forward_ws there: the one intended difference, DESIGN.md.)"""
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp)
        from m3d.model import DetectorM3D
        from m3d.prm import PRMEngine
        seen = 0
        for net, env in itertools.product(NETS, ENVS):
            set_env(mp, env)
            prm = PRMEngine(DetectorM3D(params(net), config(net)))
            rec.take()
            prm.forward_response(torch.empty((1, 1) + HUGE, device="meta"))
            for launch in rec.take()[0]:
                if launch[0].startswith("m3d_conv3d_") and "split_sigmoid" not in launch[0] and "stem" not in launch[0] and "bound_of" not in launch[0]:
                    big = item_bytes(launch) >= GUARD
                    seen += big
                    assert not (big and ("wino" in launch[0] or "zw" in launch[0])), (net, env, launch)
        assert seen >= len(NETS) * len(ENVS)


def wino2_plan(L, local, batch, cin, cout, d, h, w):
    """(return code, [family, tile id, K split]) of m3d_conv3d_wino2_plan"""
    fam, tile, ks = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = L.m3d_conv3d_wino2_plan(local, batch, cin, cout, d, h, w, C.byref(fam), C.byref(tile), C.byref(ks))
    return rc, [fam.value, tile.value, ks.value]


def wino2_plan_table(L, stem_pack_bytes=None):
    """what the library `L` answers over the plan grid: {"plans": [[batch, cin, cout, D, H = W, plan, local plan, score, local score,
    workspace bytes, local workspace bytes], ...], "stem_pack_bytes": [[cout, bytes], ...]}; scores are the library's doubles"""
    rows = []
    for batch, (cin, cout), d, hw in itertools.product(BATCHES, PLAN_LAYERS, PLAN_DEPTHS, PLAN_WIDTHS):
        a = (batch, cin, cout, d, hw, hw)
        plans = []
        for local in (0, 1):
            rc, plan = wino2_plan(L, local, *a)
            assert rc == 0, (local, a, rc)
            plans.append(plan)
        rows.append([batch, cin, cout, d, hw] + plans + [L.m3d_conv3d_wino2_score(*a), L.m3d_conv3d_wino2_local_score(*a),
                                                        L.m3d_conv3d_wino2_workspace_bytes(*a), L.m3d_conv3d_wino2_local_workspace_bytes(*a)])
    stem = stem_pack_bytes or L.m3d_conv3d_stem_wino_packed_weight_bytes
    return json.loads(json.dumps({"plans": rows, "stem_pack_bytes": [[c, stem(c)] for c in STEM_COUTS]}))


def test_wino2_plan_table_matches_the_record():
    """tile choice, split-K plan, scores (exactly: the same double arithmetic) and workspace sizes of both 2-D Winograd families, and
    the size of the stem's weight pack, as recorded before the A/B-only families and the one-row stem kernel were retired"""
    import __graft_entry__ as g
    g.build()
    from m3d import _lib
    with gzip.open(PLAN_FIXTURE, "rt") as f:
        want = json.load(f)
    assert len(want["plans"]) == len(BATCHES) * len(PLAN_LAYERS) * len(PLAN_DEPTHS) * len(PLAN_WIDTHS)
    L = _lib.lib()
    assert not L.m3d_tuning_build()
    got = wino2_plan_table(L)
    for g_row, w_row in zip(got["plans"], want["plans"]):
        assert g_row == w_row
    assert got == want


def test_wino2_option_names_family_2_or_4_and_nothing_else():
    """tune_wino2 of the tuning build: 299 runs the F(2x2) family behind the default entry points, 499 and -1 the default F(2x4); any
    other value is refused by the plan and scores / sizes 0.  No device call."""
    import __graft_entry__ as g
    g.build()
    from m3d import _lib
    a = (1, 64, 64, 32, 32, 32)
    with _lib.tuning():
        L = _lib.lib()
        assert L.m3d_tuning_build()
        default, local = wino2_plan(L, 0, *a), wino2_plan(L, 1, *a)
        assert default[0] == 0 and local[0] == 0 and default[1][0] == 4 and local[1][0] == 2
        assert L.m3d_conv3d_wino2_score(*a) > 0 and L.m3d_conv3d_wino2_local_score(*a) > 0
        for bad in (0, 3, 199, 399, 599):
            _lib.set_option("tune_wino2", bad)
            for loc in (0, 1):
                assert L.m3d_conv3d_wino2_plan(loc, *a, None, None, None) == M3D_EUNSUPPORTED, (bad, loc)
            assert L.m3d_conv3d_wino2_score(*a) == 0.0 and L.m3d_conv3d_wino2_workspace_bytes(*a) == 0, bad
            assert L.m3d_conv3d_wino2_family() == 0, bad
        _lib.set_option("tune_wino2", 299)
        assert wino2_plan(L, 0, *a) == local and L.m3d_conv3d_wino2_family() == 2
        assert L.m3d_conv3d_wino2_score(*a) == L.m3d_conv3d_wino2_local_score(*a)
        for same in (499, -1):
            _lib.set_option("tune_wino2", same)
            assert wino2_plan(L, 0, *a) == default and wino2_plan(L, 1, *a) == local and L.m3d_conv3d_wino2_family() == 4
    assert _lib.get_option("tune_wino2") == -1
