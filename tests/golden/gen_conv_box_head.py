"""Golden vectors for the conv box head: builds the REFERENCE's own `modeling.fast_rcnn_heads.roi_Xconv1fc_head` and
`fast_rcnn_outputs` on the CPU through oracle/ref_harness.py, with a stub `roi_xform_func` that returns the pooled tensor it is given,
and writes tests/golden/conv_box_head.npz: the parameter names and shapes of the two modules under the detector's prefixes
(Box_Head. / Box_Outs.), seeded weights, a seeded pooled input [R, dim_in, 7, 7, 7] and the fp32 outputs in training mode (class
scores as logits).  Arrays and names only.

Shape: dim_in 8, CONV_HEAD_DIM 8, NUM_STACKED_CONVS 2, MLP_HEAD_DIM 8, 2 classes, R = 3.

The generator asserts what the test relies on: the recorded fp32 output differs from its own fp64 evaluation (e_fixture > 0, so that
`e_module <= 4 e_fixture` is a condition an fp32 evaluation can meet) and m3d.ConvBoxHead with these weights meets it.

Run in the build container only, after oracle/build_ref.sh:  python tests/golden/gen_conv_box_head.py"""
import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

NUC = "configs/cell_tracking_baseline/e2e_mask_rcnn_N3DH_SIM_dsn_body.yaml"
DIM_IN, DIM, CONVS, MLP, CLASSES, R, RES = 8, 8, 2, 8, 2, 3, 7
OUT = os.path.join(HERE, "conv_box_head.npz")


def rel_err(outs, outs64):
    """largest |out - out64| / largest |out64| over cls_score and bbox_pred"""
    num = max(float((a.double() - b).abs().max()) for a, b in zip(outs, outs64))
    return num / max(float(b.abs().max()) for b in outs64)


def main():
    import ref_harness as H
    H.install()
    import torch
    H.load_cfg(NUC, ("FAST_RCNN.ROI_BOX_HEAD", "fast_rcnn_heads.roi_Xconv1fc_head", "FAST_RCNN.CONV_HEAD_DIM", DIM,
                     "FAST_RCNN.NUM_STACKED_CONVS", CONVS, "FAST_RCNN.MLP_HEAD_DIM", MLP, "MODEL.NUM_CLASSES", CLASSES,
                     "FAST_RCNN.ROI_XFORM_RESOLUTION", RES))
    import modeling.fast_rcnn_heads as FH
    head = FH.roi_Xconv1fc_head(DIM_IN, lambda x, rpn_ret, **kw: x, 0.125)
    outs = FH.fast_rcnn_outputs(head.dim_out)
    head.train(), outs.train()
    g = torch.Generator().manual_seed(20)
    with torch.no_grad():
        for m in (head, outs):
            for p in m.parameters():
                p.copy_(torch.randn(p.shape, generator=g) * (0.3 if p.dim() > 1 else 0.1))
    pooled = torch.randn((R, DIM_IN, RES, RES, RES), generator=g)
    with torch.no_grad():
        cls_score, bbox_pred = outs(head(pooled, None))
        h64, o64 = copy.deepcopy(head).double(), copy.deepcopy(outs).double()
        want64 = o64(h64(pooled.double(), None))
    assert cls_score.dtype == torch.float32 and tuple(cls_score.shape) == (R, CLASSES) and tuple(bbox_pred.shape) == (R, 6 * CLASSES)
    e_fixture = rel_err((cls_score, bbox_pred), want64)
    assert 0 < e_fixture < 1e-5, e_fixture
    state = {"Box_Head." + k: v for k, v in head.state_dict().items()}
    state.update({"Box_Outs." + k: v for k, v in outs.state_dict().items()})
    names = list(state)
    arrays = {"names": np.array(names), "shapes": np.array([",".join(str(d) for d in state[k].shape) for k in names]),
              "pooled": pooled.numpy(), "cls_score": cls_score.numpy(), "bbox_pred": bbox_pred.numpy(),
              "dims": np.array([DIM_IN, DIM, CONVS, MLP, CLASSES, R, RES], np.int64)}
    for k in names:
        arrays["w::" + k] = state[k].numpy()
    # the module this fixture is for meets the test's condition on it
    import m3d
    mod = m3d.ConvBoxHead(DIM_IN, 8, num_classes=CLASSES, conv_head_dim=DIM, num_stacked_convs=CONVS, mlp_head_dim=MLP, roi_res=RES)
    assert {k: tuple(v.shape) for k, v in mod.detector_state().items()} == {k: tuple(v.shape) for k, v in state.items()}
    mod.load_detector_state(state)
    with torch.no_grad():
        got = mod.trunk(pooled)
        got64 = copy.deepcopy(mod).double().trunk(pooled.double())
    e_module = rel_err(got, got64)
    print("e_fixture %.3g e_module %.3g" % (e_fixture, e_module))
    assert e_module <= 4 * e_fixture
    np.savez_compressed(OUT, **arrays)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))
    assert os.path.getsize(OUT) < 256 * 1024


if __name__ == "__main__":
    main()
