"""GPU: the conv box head (roi_Xconv1fc_head, lib/modeling/fast_rcnn_heads.py:120-179) in training, inference and end to end.
 (a) m3d.ConvBoxHead under compat.install(): every parameter gradient and the feature-map gradient against the same module in fp64 on
     the CPU, e_m3d <= 4 e_torch (the margin of test_gpu_conv_dilated.py's MaskHead check), with the narrow wgrad switch off and on;
     the launch record says which wgrad kernel ran; no conv falls through to torch;
 (b) DetectorM3D.box_head_outputs with such a checkpoint for R = 0, 7, 40 against an fp64 evaluation that starts from the library's own
     RoIAlign output, e <= 4 e_torch for cls and pred_boxes; a checkpoint that disagrees with cfg raises before anything is launched;
 (c) Generalized_RCNN / im_detect_all / PeakResponseMapping_3d on such a checkpoint; a state saved by m3d.save_ckpt from
     ConvBoxHead.detector_state() runs in DetectorM3D.
On one MI355X: (a) e_torch = 1.63e-6, e_m3d = 1.81e-6 (switch off) and 1.09e-6 (on); (b) cls e = 9.7e-7 against e_torch = 5.8e-7 at
R = 40, pred_boxes 7.7e-8 against 8.7e-8."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HEAD = "roi_Xconv1fc_head"


class Record:
    """the library object with every call written down by name and passed on (the boundary tests/test_conv_dispatch.py records at)"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def _head_fp64(head, feat, rois7, r1, r2, scale, ratio):
    """the module in fp64 on the CPU.  RoIAlign3D forward: the fp64 linear map of tests/f16x2_contract.py; its backward: the fp64 reference
    of tests/roi_align_backward_cases.py (the reference's backward kernel is not the transpose of its forward, and the library reproduces
    both)."""
    import roi_align_backward_cases as RB
    from f16x2_contract import roi_align_ref
    h = copy.deepcopy(head).cpu().double()
    x = roi_align_ref(feat.detach().cpu().double(), rois7.cpu(), scale, ratio).requires_grad_(True)
    cls, bbox = h.trunk(x)
    ((cls * r1.cpu().double()).sum() + (bbox * r2.cpu().double()).sum()).backward()
    g = {k: p.grad for k, p in h.named_parameters()}
    g["feat"] = torch.from_numpy(RB.reference(x.grad.numpy(), rois7.cpu().numpy(), tuple(feat.shape), (7, 7, 7), scale, ratio).grad)
    return g


def _grads(head, feat, rois7, r1, r2):
    for p in head.parameters():
        p.grad = None
    f = feat.clone().requires_grad_(True)
    cls, bbox = head(f, rois7)
    ((cls * r1).sum() + (bbox * r2).sum()).backward()
    got = {k: p.grad.clone() for k, p in head.named_parameters()}
    got["feat"] = f.grad
    return got


def _err(got, g64):
    assert set(got) == set(g64)
    return max(float((got[k].double().cpu() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64)


def test_training_step_on_the_library(monkeypatch):
    import m3d
    import m3d.compat as compat
    from m3d import ops
    stride = 4
    torch.manual_seed(11)
    head = m3d.ConvBoxHead(16, stride, conv_head_dim=32, num_stacked_convs=2, mlp_head_dim=32).cuda()
    with torch.no_grad():
        head.cls_score.weight.normal_(0, 0.05), head.bbox_pred.weight.normal_(0, 0.05)
        for p in head.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    gen = torch.Generator().manual_seed(12)
    feat = torch.randn((1, 16, 8, 16, 16), generator=gen).cuda()
    # (x1, y1, z1, x2, y2, z2) in image voxels of the 32 x 64 x 64 tile: a box of a few voxels (bins far below one feature voxel), one
    # that touches the border on three faces, two ordinary ones, and the zero box of a padding row, as BoxHeadTargets.rois7 pads
    rois7 = torch.tensor([[0, 20.0, 22.0, 9.0, 26.5, 27.0, 13.0],
                          [0, 40.0, 30.0, 12.0, 63.0, 63.0, 31.0],
                          [0, 3.5, 8.0, 2.0, 30.0, 41.0, 20.0],
                          [0, 10.0, 5.0, 14.0, 50.0, 33.0, 29.0],
                          [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]).cuda()
    r1, r2 = torch.randn((5, 2), generator=gen).cuda(), torch.randn((5, 12), generator=gen).cuda()
    g64 = _head_fp64(head, feat, rois7, r1, r2, 1.0 / stride, 2)
    assert all(float(v.abs().max()) > 0 for v in g64.values())
    was_installed = (compat._orig_conv3d is not None, compat._orig_linear is not None)
    compat.uninstall_conv3d(), compat.uninstall_linear()
    e_torch = _err(_grads(head, feat, rois7, r1, r2), g64)              # torch's own conv3d / linear on the device (RoIAlign: the library's)
    switches = (compat.get_conv_wgrad_narrow(), compat.get_conv_wgrad(), compat.get_conv_train(), compat.get_roi_align_backward())
    compat.install()
    try:
        def refuse(*a, **k):
            raise AssertionError("a conv of the head fell through to torch's conv3d")
        monkeypatch.setattr(compat, "_orig_conv3d", refuse)
        rec = Record(ops.lib())
        monkeypatch.setattr(ops, "lib", lambda: rec)
        e, wgrads = {}, {}
        for narrow in (False, True):
            assert compat.set_conv_wgrad_narrow(narrow) is False         # the previous value: the default, then the first round's
            rec.calls = []
            e[narrow] = _err(_grads(head, feat, rois7, r1, r2), g64)
            wgrads[narrow] = [c for c in rec.calls if c in ("m3d_conv3d_wgrad", "m3d_conv3d_wgrad_narrow", "m3d_conv3d_wgrad_f16x2")]
            assert rec.calls.count("m3d_conv3d_forward") >= 4           # two forwards and two dgrads on the direct kernel
            assert rec.calls.count("m3d_conv3d_bias_grad") == 2 and "m3d_roi_align3d_backward" in rec.calls
            assert rec.calls.count("m3d_linear_wgrad") == 3
        print("ConvBoxHead gradients: e_torch %.3g e_m3d %.3g (narrow off) %.3g (narrow on)" % (e_torch, e[False], e[True]))
        assert wgrads[False] == ["m3d_conv3d_wgrad"] * 2 and wgrads[True] == ["m3d_conv3d_wgrad_narrow"] * 2
        assert e[False] <= 4 * e_torch, (e, e_torch)
        assert e[True] <= 4 * e_torch, (e, e_torch)
    finally:
        monkeypatch.undo()
        compat.set_conv_wgrad_narrow(switches[0]), compat.set_conv_wgrad(switches[1]), compat.set_conv_train(switches[2])
        compat.set_roi_align_backward(switches[3])
        compat.uninstall_conv3d(), compat.uninstall_linear()
        if was_installed[0]:
            compat.install_conv3d()
        if was_installed[1]:
            compat.install_linear()
    assert compat.get_conv_wgrad_narrow() is switches[0]


# ------------------------------------------------------------------------------------------------------------- inference
def _cfg(**kw):
    from m3d.config import Cfg
    return Cfg.nuclei(**dict(dict(mlp_dim=64, box_head=HEAD, conv_head_dim=32, num_stacked_convs=2, score_thresh=0.0), **kw))


def _params(seed=5, **kw):
    from m3d.synth import make_params
    P = make_params(**dict(dict(stride=8, num_anchors=35, mlp_dim=64, seed=seed, box_head=HEAD, conv_head_dim=32, num_stacked_convs=2), **kw))
    return {k: v.cuda() for k, v in P.items()}


def _decode(rois, deltas, weights):
    """lib/utils/boxes_3d.py:167-225 in the dtype of its arguments"""
    from m3d.config import BBOX_XFORM_CLIP
    b = rois[:, 1:7]
    size = b[:, 3:6] - b[:, 0:3] + 1.0
    ctr = b[:, 0:3] + 0.5 * size
    d = deltas.reshape(deltas.shape[0], -1, 6) / torch.tensor(weights, dtype=deltas.dtype, device=deltas.device)
    pc = d[:, :, 0:3] * size[:, None] + ctr[:, None]
    ps = torch.exp(torch.clamp(d[:, :, 3:6], max=BBOX_XFORM_CLIP)) * size[:, None]
    return torch.cat([pc - 0.5 * ps, pc + 0.5 * ps - 1.0], 2).reshape(deltas.shape)


def _compose(P, x, rois, cfg, dtype, device):
    """convs -> fc -> outs -> softmax / decode from the RoIAlign output x, in `dtype` on `device`"""
    t = lambda v: v.to(device=device, dtype=dtype)
    x = t(x)
    for i in range(cfg.num_stacked_convs):
        x = torch.relu(F.conv3d(x, t(P["Box_Head.convs.%d.weight" % (2 * i)]), t(P["Box_Head.convs.%d.bias" % (2 * i)]), 1, 1))
    x = torch.relu(F.linear(x.flatten(1), t(P["Box_Head.fc.weight"]), t(P["Box_Head.fc.bias"])))
    cls = torch.softmax(F.linear(x, t(P["Box_Outs.cls_score.weight"]), t(P["Box_Outs.cls_score.bias"])), 1)
    bbox = F.linear(x, t(P["Box_Outs.bbox_pred.weight"]), t(P["Box_Outs.bbox_pred.bias"]))
    return cls, bbox, _decode(t(rois), bbox, cfg.bbox_reg_weights)


def _rois(R, gen):
    lo = torch.rand((R, 3), generator=gen) * torch.tensor([40.0, 40.0, 18.0])
    hi = lo + 2.0 + torch.rand((R, 3), generator=gen) * torch.tensor([22.0, 22.0, 12.0])
    return torch.cat([torch.randint(0, 2, (R, 1), generator=gen).float(), lo, hi], 1).cuda()


def test_box_head_outputs_of_the_detector():
    from m3d import ops
    from m3d.model import DetectorM3D
    cfg, P = _cfg(), _params()
    det = DetectorM3D(P, cfg)
    assert det.conv_head and det.has_head and len(det.head_convs) == 2
    gen = torch.Generator().manual_seed(6)
    feat = torch.randn((2, 256, 4, 8, 8), generator=gen).cuda()
    for R in (0, 7, 40):
        rois = _rois(R, gen)
        cls, bbox, pred = det.box_head_outputs(feat, rois)
        assert cls.shape == (R, 2) and bbox.shape == (R, 12) and pred.shape == (R, 12) and cls.dtype == torch.float32
        assert det.box_head(feat, rois)[0].shape == (R, 2)
        if R == 0:
            continue
        x = ops.roi_align3d_forward(feat, rois, 7, 7, 7, 1.0 / 8, 2)
        c64, b64, p64 = _compose(P, x, rois, cfg, torch.float64, "cpu")
        c32, b32, p32 = _compose(P, x, rois, cfg, torch.float32, "cuda")
        for name, got, t32, ref in (("cls", cls, c32, c64), ("pred_boxes", pred, p32, p64)):
            e = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
            e_torch = float((t32.double().cpu() - ref).abs().max() / ref.abs().max())
            print("R %2d %-10s e %.3g e_torch %.3g" % (R, name, e, e_torch))
            assert e <= 4 * e_torch, (R, name, e, e_torch)
        assert float((bbox.double().cpu() - b64).abs().max()) <= 1e-4 * float(b64.abs().max())
        assert float(cls.sum(1).sub(1).abs().max()) < 1e-5
    # clip_to reaches the boxes as on the two-FC path
    pc = det.box_head_outputs(feat, rois, clip_to=(32, 64, 64))[2]
    assert float(pc.min()) >= 0 and float(pc[:, 0::3].max()) <= 63 and float(pc[:, 2::3].max()) <= 31


def test_a_checkpoint_that_disagrees_with_cfg_raises_before_anything_is_launched(monkeypatch):
    from m3d import ops
    from m3d.model import DetectorM3D
    P = _params()

    def no_launch():
        raise AssertionError("the library was reached before the check")
    monkeypatch.setattr(ops, "lib", no_launch)
    three = dict(P)
    three["Box_Head.convs.4.weight"], three["Box_Head.convs.4.bias"] = P["Box_Head.convs.2.weight"], P["Box_Head.convs.2.bias"]
    no_fc = {k: v for k, v in P.items() if not k.startswith("Box_Head.fc.")}
    for params, cfg in ((P, _cfg(num_stacked_convs=3)), (P, _cfg(num_stacked_convs=1)), (three, _cfg()), (P, _cfg(conv_head_dim=64)),
                        (P, _cfg(mlp_dim=32)), (P, _cfg(roi_res=5)), (no_fc, _cfg())):
        with pytest.raises(ValueError):
            DetectorM3D(params, cfg)


# ------------------------------------------------------------------------------------------------------------- end to end
def test_drivers_and_prm_on_a_conv_head_checkpoint():
    from m3d.drivers import Generalized_RCNN, PeakResponseMapping_3d, im_detect_all
    from m3d.synth import synth_volume, unsaturated_rpn
    cfg = _cfg(in_size=(32, 64, 64), crop_ovlp=8)
    P = unsaturated_rpn(_params(seed=9))
    im = synth_volume(0, (32, 64, 64))
    model = Generalized_RCNN({"model": P}, cfg)
    assert model.det.conv_head
    cls_boxes, cls_segms, cls_keyps = im_detect_all(model, im)
    assert cls_keyps is None and cls_segms == [[], []] and cls_boxes[0].shape == (0, 7)
    assert cls_boxes[1].dtype == np.float32 and cls_boxes[1].shape[1] == 7 and cls_boxes[1].shape[0] > 0
    assert np.isfinite(cls_boxes[1]).all() and (cls_boxes[1][:, 6] >= 0).all() and (cls_boxes[1][:, 6] <= 1).all()
    vol = ((im - im.mean()) / im.std()).astype(np.float32)
    blobs = {"data": [torch.from_numpy(vol[None, None])], "im_info": [torch.from_numpy(np.array([[32, 64, 64, 1.0]]))]}
    rd = model(**blobs)
    R = rd["rois"].shape[0]
    assert R > 0 and rd["cls_score"].shape == (R, 2) and rd["bbox_pred"].shape == (R, 12) and torch.isfinite(rd["cls_score"]).all()
    # PRM: each peak's value is the box-head score of its detection
    pm = PeakResponseMapping_3d({"model": P}, cfg).inference()
    seen, orig = [], pm.det.box_head_outputs
    pm.det.box_head_outputs = lambda *a, **k: (seen.append(orig(*a, **k)), seen[-1])[1]
    scores = torch.sort(rd["_m3d"]["det_scores"])[0]
    thr = float(scores[len(scores) // 2]) if len(scores) > 1 else 0.0                  # about half of the detections become peaks
    res = pm(peak_threshold=thr, im_scale=[1.0], **blobs)
    assert len(res) == 5 and res[0] is None and res[4] is not None and len(seen) == 1
    _, crm, peaks, prms, dets = res
    assert dets.dtype == torch.float64 and dets.shape == (peaks.shape[0], 7) and prms.shape == (peaks.shape[0], 32, 64, 64)
    head_scores = set(seen[0][0][:, 1].double().cpu().tolist())
    assert dets.shape[0] > 0 and all(v in head_scores and v > thr for v in dets[:, 6].cpu().tolist())
    assert torch.isfinite(prms).all()


def test_a_trained_state_runs_in_the_detector(tmp_path):
    import m3d
    from m3d import ops
    from m3d.drivers import _to_params
    from m3d.model import DetectorM3D
    cfg, P = _cfg(), _params(head=False)
    torch.manual_seed(3)
    head = m3d.ConvBoxHead(256, 8, conv_head_dim=32, num_stacked_convs=2, mlp_head_dim=64).cuda()
    with torch.no_grad():
        head.cls_score.weight.normal_(0, 0.05), head.bbox_pred.weight.normal_(0, 0.05)

    class Net(torch.nn.Module):                                          # the detector's state dict: body + RPN + the head's
        def __init__(self):
            super().__init__()
            self.head = head

        def state_dict(self, *a, **k):
            return dict(P, **head.detector_state())
    solver = m3d.Solver(head.named_parameters(), m3d.SolverCfg())
    bias_group = solver.param_groups[1]["params"]
    assert len(bias_group) == 5 and all(p.dim() == 1 for p in bias_group)            # two convs, fc, cls_score, bbox_pred
    assert len(solver.param_groups[0]["params"]) == 5
    path = m3d.save_ckpt(str(tmp_path), 0, Net(), solver)
    ckpt = torch.load(path, map_location="cpu")
    assert {"Box_Head.convs.0.weight", "Box_Head.convs.2.bias", "Box_Head.fc.weight", "Box_Outs.bbox_pred.bias"} <= set(ckpt["model"])
    det = DetectorM3D(_to_params(ckpt, torch.device("cuda")), cfg)
    assert det.conv_head
    again = m3d.ConvBoxHead(256, 8, conv_head_dim=32, num_stacked_convs=2, mlp_head_dim=64)
    again.load_detector_state(ckpt["model"])
    assert all(torch.equal(a, b.cpu()) for a, b in zip(again.state_dict().values(), head.state_dict().values()))
    gen = torch.Generator().manual_seed(4)
    feat = torch.randn((2, 256, 4, 8, 8), generator=gen).cuda()
    rois = _rois(40, gen)
    cls = det.box_head_outputs(feat, rois)[0]
    x = ops.roi_align3d_forward(feat, rois, 7, 7, 7, 1.0 / 8, 2)
    with torch.no_grad():
        want = torch.softmax(head.trunk(x)[0], 1)                        # the module on the device, torch's own arithmetic
        ref = torch.softmax(copy.deepcopy(head).cpu().double().trunk(x.cpu().double())[0], 1)
    e = float((cls.double().cpu() - ref).abs().max() / ref.abs().max())
    e_torch = float((want.double().cpu() - ref).abs().max() / ref.abs().max())
    print("trained state in DetectorM3D: e %.3g e_torch %.3g" % (e, e_torch))
    assert e <= 4 * e_torch, (e, e_torch)
