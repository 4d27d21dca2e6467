"""CPU: the conv box head (roi_Xconv1fc_head, lib/modeling/fast_rcnn_heads.py:120-179) on the host side - Cfg.from_yaml's three keys and
its refusals; the C ABI of m3d_conv3d_wgrad_narrow* refuses what it must before any pointer is followed or anything is launched, so
every call below is safe with made-up pointers on a machine without a GPU; conv_plan.wgrad_kernel's `narrow` keyword and the compat
switch; m3d.ConvBoxHead's parameter names, shapes and arithmetic against tests/golden/conv_box_head.npz, which
tests/golden/gen_conv_box_head.py recorded from the reference's own module."""
import copy
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import conv_wgrad_narrow_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_box_head.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


# the keys of this path as the two shipped YAMLs write them (nuclei: stride 8 with the conv-head numbers set; soma: stride 4 without)
_YAML = """
MODEL:
  TYPE: generalized_rcnn
  CONV_BODY: DSN.dsn_body
  NUM_CLASSES: 2
  BBOX_REG_WEIGHTS: (10., 10., 10., 5., 5., 5.)
RPN:
  STRIDE: %(stride)d
  SIZES: (10, 27, 33)
  ASPECT_RATIOS: [[1.0, 0.5]]
FAST_RCNN:
  ROI_BOX_HEAD: %(head)s
  ROI_XFORM_METHOD: RoIAlign
  ROI_XFORM_RESOLUTION: 7
  ROI_XFORM_SAMPLING_RATIO: 2
  MLP_HEAD_DIM: 1024
%(extra)s"""
_NUMBERS = "  CONV_HEAD_DIM: 128 # default 256\n  NUM_STACKED_CONVS: 2 #default 4\n"


def test_cfg_from_yaml():
    from m3d.config import Cfg
    for head in ("fast_rcnn_heads.roi_Xconv1fc_head", "roi_Xconv1fc_head"):
        c = Cfg.from_yaml(_YAML % dict(stride=8, head=head, extra=_NUMBERS))
        assert (c.box_head, c.conv_head_dim, c.num_stacked_convs) == ("roi_Xconv1fc_head", 128, 2)
        c = Cfg.from_yaml(_YAML % dict(stride=8, head=head, extra=""))
        assert (c.box_head, c.conv_head_dim, c.num_stacked_convs) == ("roi_Xconv1fc_head", 256, 4)        # lib/core/config.py:637,639
    for head in ("fast_rcnn_heads.roi_2mlp_head", "roi_2mlp_head"):
        assert Cfg.from_yaml(_YAML % dict(stride=8, head=head, extra=_NUMBERS)).box_head == "roi_2mlp_head"
    assert Cfg.from_yaml(_YAML.replace("  ROI_BOX_HEAD: %(head)s\n", "") % dict(stride=4, extra="")).box_head == "roi_2mlp_head"
    with pytest.raises(NotImplementedError, match="2-D"):
        Cfg.from_yaml(_YAML % dict(stride=8, head="fast_rcnn_heads.roi_Xconv1fc_gn_head", extra=_NUMBERS))
    for head in ("fast_rcnn_heads.roi_2mlp_head_gn", "ResNet.ResNet_roi_conv5_head", "roi_Xconv1fc"):
        with pytest.raises(NotImplementedError):
            Cfg.from_yaml(_YAML % dict(stride=8, head=head, extra=""))
    # the defaults, and the two shipped files as they are written (nuclei sets the two numbers, soma neither)
    assert (Cfg().box_head, Cfg.nuclei().box_head, Cfg.soma().box_head) == ("roi_2mlp_head",) * 3
    n = Cfg.from_yaml(_YAML % dict(stride=8, head="fast_rcnn_heads.roi_2mlp_head", extra=_NUMBERS))
    s = Cfg.from_yaml(_YAML % dict(stride=4, head="fast_rcnn_heads.roi_2mlp_head", extra=""))
    for got, want in ((n, Cfg.nuclei()), (s, Cfg.soma())):
        assert (got.box_head, got.conv_head_dim, got.num_stacked_convs) == (want.box_head, want.conv_head_dim, want.num_stacked_convs)
    base = os.path.join(os.environ.get("M3D_REFERENCE", "/root/reference"), "configs")
    if os.path.isdir(base):                                            # read where the reference lies, when it is there
        for rel, want in (("cell_tracking_baseline/e2e_mask_rcnn_N3DH_SIM_dsn_body.yaml", Cfg.nuclei()),
                          ("soma_starting/e2e_mask_rcnn_soma_dsn_body.yaml", Cfg.soma())):
            got = Cfg.from_yaml(os.path.join(base, rel))
            assert (got.box_head, got.conv_head_dim, got.num_stacked_convs) == ("roi_2mlp_head", want.conv_head_dim, want.num_stacked_convs)


# ----------------------------------------------------------------------------------------------- the narrow wgrad's ABI
X, GY, GW, WS = 0x100000, 0x200000, 0x300000, 0x400000
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
DIMS = dict(batch=3, cin=32, cout=32, D=7, H=7, W=7, k=3)


def p(v):
    return C.c_void_p(v)


def need(L, **kw):
    d = dict(DIMS, **kw)
    return L.m3d_conv3d_wgrad_narrow_workspace_bytes(*[d[k] for k in DIMS])


def supported(L, **kw):
    d = dict(DIMS, **kw)
    return L.m3d_conv3d_wgrad_narrow_supported(*[d[k] for k in DIMS])


def plan(L, **kw):
    d = dict(DIMS, **kw)
    v = [C.c_int(-1) for _ in range(3)]
    rc = L.m3d_conv3d_wgrad_narrow_plan(*[d[k] for k in DIMS], *[C.byref(a) for a in v])
    return rc, tuple(a.value for a in v)


def wgrad(L, x=X, gy=GY, gw=GW, ws=WS, wsb=None, **kw):
    d = dict(DIMS, **kw)
    wsb = need(L, **kw) if wsb is None else wsb
    return L.m3d_conv3d_wgrad_narrow(p(x), p(gy), p(gw), *[d[k] for k in DIMS], p(ws), C.c_size_t(wsb), None)


def test_abi_limits_without_a_gpu(L):
    from m3d._lib import SYMBOLS
    for s in ("m3d_conv3d_wgrad_narrow_workspace_bytes", "m3d_conv3d_wgrad_narrow", "m3d_conv3d_wgrad_narrow_supported",
              "m3d_conv3d_wgrad_narrow_plan"):
        assert s in SYMBOLS and hasattr(L, s), s
    assert need(L) > 0 and supported(L) == 1 and plan(L)[0] == 0
    # M3D_EINVAL: NULL pointers, non-positive extents
    for k in ("x", "gy", "gw", "ws"):
        assert wgrad(L, **{k: None}) == EINVAL, k
    for k in ("batch", "cin", "cout", "D", "H", "W"):
        for v in (0, -3):
            assert wgrad(L, wsb=1 << 20, **{k: v}) == EINVAL, (k, v)
            assert need(L, **{k: v}) == 0 and supported(L, **{k: v}) == 0 and plan(L, **{k: v})[0] == EINVAL
    # M3D_EWORKSPACE: a short workspace
    assert wgrad(L, wsb=need(L) - 1) == EWORKSPACE and wgrad(L, wsb=0) == EWORKSPACE
    # M3D_EUNSUPPORTED: k != 3, a map wider than 8, one image of x or gy beyond the 32-bit offsets, 2^31 tiles
    for kw in (dict(k=1), dict(k=5), dict(k=5, cin=1), dict(k=2), dict(W=9), dict(W=16), dict(W=1 << 20),
               dict(batch=1, cin=1, cout=1, D=1 << 14, H=1 << 13, W=4), dict(batch=1, cin=1 << 13, cout=1, D=1 << 7, H=1 << 6, W=8),
               dict(batch=1, cin=1, cout=1 << 13, D=1 << 7, H=1 << 6, W=8), dict(batch=1 << 30, D=8, H=8, W=8)):
        assert wgrad(L, wsb=1 << 20, **kw) == EUNSUPPORTED, kw
        assert need(L, **kw) == 0 and supported(L, **kw) == 0 and plan(L, **kw)[0] == EUNSUPPORTED, kw
    # just inside the limits: W = 8, an image one float short of the limit
    assert supported(L, W=8) == 1 and supported(L, batch=1, cin=1, cout=1, D=(1 << 26) - 1, H=1, W=8) == 1
    assert supported(L, batch=1, cin=1, cout=1, D=1 << 26, H=1, W=8) == 0


def test_workspace_and_plan(L):
    for case in T.CASES + [(128, 256, 128, 7, 7, 7), (512, 128, 128, 7, 7, 7), (300, 256, 256, 7, 7, 7), (16, 256, 256, 7, 7, 7)]:
        B, cin, cout, D, H, W = case
        kw = dict(batch=B, cin=cin, cout=cout, D=D, H=H, W=W)
        rc, (tx, ty, slots) = plan(L, **kw)
        assert rc == 0 and (tx, ty) == (8, 8)
        tiles = B * -(-D // 2) * -(-H // 8)
        assert 1 <= slots <= tiles                                                              # no slot without a tile
        assert need(L, **kw) >= slots * cout * cin * 27 * 4
        assert plan(L, **kw) == (rc, (tx, ty, slots))                                           # a function of the shape only
        assert L.m3d_conv3d_wgrad_narrow_plan(B, cin, cout, D, H, W, 3, None, None, None) == 0  # any output pointer may be NULL
        # the slot count does not depend on the width (one tile along x)
        assert all(plan(L, **dict(kw, W=w))[1][2] == slots for w in (1, 8))
    assert plan(L, batch=1, cin=4, cout=5, D=2, H=8, W=8)[1][2] == 1
    # the other wgrad entry points keep their refusals: dilation 1 is not the dilated kernel's
    assert L.m3d_conv3d_wgrad_dilated_plan(1, 4, 5, 2, 8, 8, 3, 1, 0, None, None, None) == EUNSUPPORTED


# ----------------------------------------------------------------------------------------------- routing
def _today(batch, cin, cout, D, H, W, mode, k=3):
    """conv_plan.wgrad_kernel as it was before the `narrow` keyword (the rule of its docstring)"""
    from m3d import conv_plan as cp, ops
    if mode == cp.WGRAD_FP32 or k != 3 or not ops.conv3d_wgrad_f16x2_supported(batch, cin, cout, D, H, W):
        return cp.WGRAD_FP32
    return cp.WGRAD_F16X2 if batch * D * H * W * cin * cout >= cp.WGRAD_F16X2_MIN_WORK else cp.WGRAD_FP32


def test_wgrad_kernel_routing(L):
    from m3d import conv_plan as cp, ops
    assert cp.WGRAD_NARROW not in (cp.WGRAD_FP32, cp.WGRAD_F16X2)
    shapes = [(b, ci, co, d, h, w) for b, (ci, co), (d, h, w) in itertools.product(
        (1, 16, 128, 512), ((32, 32), (256, 128), (128, 128), (256, 256), (33, 31), (4, 5), (16, 32)),
        ((7, 7, 7), (8, 8, 8), (14, 14, 14), (7, 7, 9), (1, 7, 7), (14, 14, 8), (16, 16, 16), (64, 64, 64), (2, 4, 16)))]
    seen = set()
    for s in shapes:
        for mode in ("fp32", "f16x2"):
            for k in (1, 3, 5):
                want = _today(*s, mode, k=k)
                assert cp.wgrad_kernel(*s, mode, k=k) == want and cp.wgrad_kernel(*s, mode, k=k, narrow=False) == want, (s, mode, k)
                takes = k == 3 and s[5] <= 8 and ops.conv3d_wgrad_narrow_supported(*s, k) and want == cp.WGRAD_FP32
                got = cp.wgrad_kernel(*s, mode, k=k, narrow=True)
                assert got == (cp.WGRAD_NARROW if takes else want), (s, mode, k, got)
                seen.add((mode, got))
    assert seen == {(m, g) for m in ("fp32", "f16x2") for g in (cp.WGRAD_FP32, cp.WGRAD_NARROW)} | {("f16x2", cp.WGRAD_F16X2)}
    # the head's and the mask head's layers
    for s in ((128, 256, 128, 7, 7, 7), (128, 128, 128, 7, 7, 7), (64, 256, 256, 7, 7, 7)):
        assert cp.wgrad_kernel(*s, "fp32", narrow=True) == cp.WGRAD_NARROW and cp.wgrad_kernel(*s, "f16x2", narrow=True) == cp.WGRAD_F16X2
    assert cp.wgrad_kernel(1, 32, 32, 7, 7, 9, "fp32", narrow=True) == cp.WGRAD_FP32
    assert cp.wgrad_kernel(1, 32, 32, 7, 7, 7, "fp32", k=1, narrow=True) == cp.WGRAD_FP32
    with pytest.raises(ValueError):
        cp.wgrad_kernel(1, 32, 32, 7, 7, 7, "bf16", narrow=True)


def test_set_conv_wgrad_narrow():
    import m3d.compat as compat
    assert compat.get_conv_wgrad_narrow() is False
    try:
        assert compat.set_conv_wgrad_narrow(True) is False and compat.get_conv_wgrad_narrow() is True
        compat.install_conv3d(), compat.install_linear()                # what install() does to F.conv3d / F.linear leaves it alone
        assert compat.get_conv_wgrad_narrow() is True
        assert compat.set_conv_wgrad_narrow(False) is True and compat.get_conv_wgrad_narrow() is False
        compat.install_conv3d(), compat.install_linear()
        assert compat.get_conv_wgrad_narrow() is False
        assert compat.set_conv_wgrad_narrow(1) is False and compat.get_conv_wgrad_narrow() is True        # any truth value
    finally:
        compat.set_conv_wgrad_narrow(False)
        compat.uninstall_conv3d(), compat.uninstall_linear()


# ----------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope="module")
def fixture():
    z = np.load(FIXTURE)
    assert os.path.getsize(FIXTURE) < 256 * 1024
    names = [str(n) for n in z["names"]]
    shapes = {n: tuple(int(v) for v in str(s).split(",")) for n, s in zip(names, z["shapes"])}
    weights = {n: torch.from_numpy(z["w::" + n]) for n in names}
    return dict(names=names, shapes=shapes, weights=weights, pooled=torch.from_numpy(z["pooled"]),
                outs=(torch.from_numpy(z["cls_score"]), torch.from_numpy(z["bbox_pred"])), dims=[int(v) for v in z["dims"]])


def _module(fixture, **kw):
    import m3d
    dim_in, dim, convs, mlp, classes, R, res = fixture["dims"]
    return m3d.ConvBoxHead(dim_in, 8, num_classes=classes, conv_head_dim=dim, num_stacked_convs=convs, mlp_head_dim=mlp, roi_res=res, **kw)


def test_module_names_shapes_and_state(fixture):
    import m3d
    from m3d.compat import RoIAlign_3d
    mod = _module(fixture)
    state = mod.detector_state()
    assert list(state) == fixture["names"]                               # the reference's keys, in the reference's order
    assert {k: tuple(v.shape) for k, v in state.items()} == fixture["shapes"]
    assert {"Box_Head.convs.0.weight", "Box_Head.convs.2.bias", "Box_Head.fc.weight", "Box_Outs.cls_score.bias",
            "Box_Outs.bbox_pred.weight"} <= set(state)
    assert isinstance(mod.roi_align, RoIAlign_3d) and isinstance(mod.convs, torch.nn.Sequential)
    assert [type(m) for m in mod.convs] == [torch.nn.Conv3d, torch.nn.ReLU] * 2
    # round trip through the detector's names
    other = _module(fixture)
    assert any(not torch.equal(a, b) for a, b in zip(other.state_dict().values(), mod.state_dict().values()))
    other.load_detector_state(dict(state, **{"Conv_Body.conv1a.weight": torch.zeros(1)}))       # keys of other parts are not its own
    assert all(torch.equal(a, b) for a, b in zip(other.state_dict().values(), mod.state_dict().values()))
    # the defaults are the nuclei YAML's; class-agnostic regression has two box columns sets
    big = m3d.ConvBoxHead(16, 8)
    assert tuple(big.fc.weight.shape) == (1024, 128 * 343) and len(big.convs) == 4 and tuple(big.bbox_pred.weight.shape) == (12, 1024)
    assert tuple(m3d.ConvBoxHead(4, 8, num_classes=3, conv_head_dim=4, num_stacked_convs=1, mlp_head_dim=8,
                                 cls_agnostic_bbox_reg=True).bbox_pred.weight.shape) == (12, 8)
    # initialisation: fc uniform +- sqrt(3 / fan_in) with zero bias; the outputs' small normal weights; conv biases are torch's (not zero)
    b = (3.0 / big.fc.in_features) ** 0.5
    assert float(big.fc.weight.detach().abs().max()) <= b and float(big.fc.weight.detach().abs().max()) > 0.99 * b and not big.fc.bias.any()
    assert 0.005 < float(big.cls_score.weight.detach().std()) < 0.02 and 0.0005 < float(big.bbox_pred.weight.detach().std()) < 0.002
    assert not big.cls_score.bias.any() and not big.bbox_pred.bias.any() and big.convs[0].bias.any()


def _rel_err(outs, outs64):
    num = max(float((a.double() - b).abs().max()) for a, b in zip(outs, outs64))
    return num / max(float(b.abs().max()) for b in outs64)


def test_trunk_against_the_reference_fixture(fixture):
    mod = _module(fixture)
    mod.load_detector_state(fixture["weights"])
    mod.train()
    with torch.no_grad():
        got = mod.trunk(fixture["pooled"])
        want64 = copy.deepcopy(mod).double().trunk(fixture["pooled"].double())
    assert [tuple(t.shape) for t in got] == [tuple(t.shape) for t in fixture["outs"]]
    e_fixture, e_module = _rel_err(fixture["outs"], want64), _rel_err(got, want64)
    print("e_fixture %.3g e_module %.3g" % (e_fixture, e_module))
    assert e_fixture > 0                                                 # the fixture alone meets the condition, and it is one
    assert _rel_err(fixture["outs"], want64) <= 4 * e_fixture
    assert e_module <= 4 * e_fixture
    # teeth: a module that drops one ReLU, or the fc's, is far outside
    with torch.no_grad():
        x = mod.convs[2](mod.convs[0](fixture["pooled"]))
        x = torch.relu(mod.fc(torch.relu(x).reshape(x.shape[0], -1)))
        assert _rel_err((mod.cls_score(x), mod.bbox_pred(x)), want64) > 4 * e_fixture
    # with F.conv3d / F.linear intercepted (what compat.install() does) CPU tensors fall through to torch: the same bits
    import m3d.compat as compat
    compat.install_conv3d(), compat.install_linear()
    try:
        assert torch.nn.functional.conv3d is compat.conv3d and torch.nn.functional.linear is compat.linear
        with torch.no_grad():
            again = mod.trunk(fixture["pooled"])
    finally:
        compat.uninstall_conv3d(), compat.uninstall_linear()
    assert all(torch.equal(a, b) for a, b in zip(again, got))
