#!/usr/bin/env python3
"""Demo: the joint RPN + box-head training step on one synthetic tile, without leaving the device between the RPN and the box-head loss.

What tools/train_rpn.py does, extended by the box head: body -> RPN head -> m3d.rpn_targets / m3d.rpn_losses;
m3d.generate_proposals3d_batched under no_grad with the TRAIN top-N settings (RPN_PRE_NMS_TOP_N 1000, RPN_POST_NMS_TOP_N 2000,
RPN_NMS_THRESH 0.7); m3d.box_head_targets on those proposals and the ground-truth boxes; RoIAlign (7^3, sampling ratio 2) -> two FC
layers -> cls_score / bbox_pred (lib/modeling/fast_rcnn_heads.py:12-47, 74-117) as plain torch.nn modules whose convolutions, linear
layers and RoIAlign run on libm3d through m3d.compat; m3d.box_head_losses; torch.optim.SGD on the sum of the four losses.
Prints all four losses per step.  One fixed sample; this is not a training driver (no data loading, schedule or checkpoints).

--mask spot (off by default; without it nothing changes) adds the mask branch: m3d.MaskHead on the same features, m3d.mask_targets from
the spheres inscribed in the synthetic boxes, m3d.mask_losses; loss_mask joins the printed line and the sum.  --mask-dilation 2 builds that head with MRCNN.DILATION = 2 (the reference's
default; both shipped YAMLs set 1), and --conv-dilated m3d runs its dilated convs on the library, forward and backward;
--conv-dilated-f16 (with --conv-dilated m3d) runs their forward and backward-data pass on the dilation-2 instantiation of the
narrow-map f16x2 kernel (m3d.compat.set_conv_dilated_f16, csrc/conv3d_zn.hip: launches of at least conv_plan.ZN_DILATED_MIN_UNITS units);
--wgrad-dilated-f16 (with --mask spot --mask-dilation 2 --conv-dilated m3d) runs their weight gradient on the dilation-2 instantiation
of the narrow-map f16x2 wgrad kernel (m3d.compat.set_conv_wgrad_dilated_f16, csrc/conv3d_wgrad_narrow_f16.hip: layers of at least
conv_plan.WGRAD_DILATED_F16X2_MIN_WORK products per tap).

--box-head conv (default mlp, whose output stays as it is) trains m3d.ConvBoxHead (roi_Xconv1fc_head, fast_rcnn_heads.py:120-179:
--conv-head-convs 3^3 convs of --conv-head-dim channels on the 7^3 grids, then one FC layer of --hidden) in place of the two-FC head;
--wgrad-narrow moves the weight gradient of every intercepted dilation-1 conv on a map at most 8 wide (those head convs and, with
--mask, the mask head's) to the 2 x 8 x 8 tile kernel (m3d.compat.set_conv_wgrad_narrow, csrc/conv3d_wgrad.hip);
--conv-narrow f16x2 runs the forward and the backward-data pass of those convs on the narrow-map f16x2 kernel
(m3d.compat.set_conv_train_narrow, csrc/conv3d_zn.hip); --wgrad-narrow-f16 runs their weight gradient on the f16 matrix cores on that
2 x 8 x 8 tile (m3d.compat.set_conv_wgrad_narrow_f16, csrc/conv3d_wgrad_narrow_f16.hip: layers of at least
conv_plan.WGRAD_NARROW_F16X2_MIN_WORK products per tap, whatever --wgrad and --wgrad-narrow say).  They compose.

--linear-backward f16x2 (default fp32) runs the backward of the FC layers on the f16 matrix cores at fp32 accuracy
(m3d.compat.set_linear_backward, csrc/fc_backward_f16.hip: layers of at least conv_plan.LINEAR_BACKWARD_F16X2_MIN_WORK M N K).

--upconv-backward f16x2 (default fp32; with --mask and --upconv m3d) runs the backward of the mask head's up-conv on the f16 matrix
cores at fp32 accuracy for the directions conv_plan.upconv_backward_kernel routes (m3d.compat.set_upconv_backward,
csrc/upconv3d_bwd_f16.hip: the dgrad from conv_plan.UPCONV_BWD_F16_MIN_DGRAD multiply-adds up; the wgrad does not route by default)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_box_head(dim_in, hidden, num_classes, stride):
    import torch.nn as nn
    import torch.nn.functional as F
    from m3d.compat import RoIAlign_3d

    class BoxHead(nn.Module):
        def __init__(self):
            super().__init__()
            self.roi_align = RoIAlign_3d(7, 7, 7, 1.0 / stride, 2)
            self.fc1, self.fc2 = nn.Linear(dim_in * 7 ** 3, hidden), nn.Linear(hidden, hidden)
            self.cls_score, self.bbox_pred = nn.Linear(hidden, num_classes), nn.Linear(hidden, 6 * num_classes)
            for m in (self.fc1, self.fc2):
                nn.init.xavier_uniform_(m.weight)
                nn.init.constant_(m.bias, 0)
            nn.init.normal_(self.cls_score.weight, std=0.01)          # fast_rcnn_heads.py:23-27
            nn.init.normal_(self.bbox_pred.weight, std=0.001)
            nn.init.constant_(self.cls_score.bias, 0)
            nn.init.constant_(self.bbox_pred.bias, 0)

        def forward(self, feat, rois7):
            x = self.roi_align(feat, rois7)
            x = F.relu(self.fc1(x.reshape(x.shape[0], -1)))
            x = F.relu(self.fc2(x))
            return self.cls_score(x), self.bbox_pred(x)
    return BoxHead()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--tile", type=int, nargs=3, default=(32, 64, 64), help="slices height width, multiples of 8")
    ap.add_argument("--width", type=int, default=16, help="channels of the first conv (the reference has 32)")
    ap.add_argument("--hidden", type=int, default=256, help="width of the two FC layers (the reference has 1024)")
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--mask", choices=("spot",), default=None, help="also train the mask branch on spheres inscribed in the boxes")
    ap.add_argument("--wgrad", choices=("fp32", "f16x2"), default="fp32",
                    help="conv weight-gradient kernel (m3d.compat.set_conv_wgrad): f16x2 = the f16 matrix cores where conv_plan.wgrad_kernel routes a layer")
    ap.add_argument("--conv", choices=("fp32", "f16x2"), default="fp32",
                    help="conv forward / backward-data kernel (m3d.compat.set_conv_train): f16x2 = the f16 matrix cores where conv_plan.train_conv_kernel routes a layer")
    ap.add_argument("--roi-backward", choices=("atomic", "ordered"), default="atomic",
                    help="RoIAlign backward kernel (m3d.compat.set_roi_align_backward) of the box head and, with --mask spot, of the mask "
                         "branch: ordered = the gather form without atomics, bit-identical from run to run")
    ap.add_argument("--upconv", choices=("torch", "m3d"), default="torch",
                    help="with --mask: the mask head's ConvTranspose3d + ReLU (m3d.compat.set_upconv): m3d = csrc/upconv3d.hip, forward and "
                         "backward, bias and ReLU fused")
    ap.add_argument("--upconv-f16", action="store_true",
                    help="with --upconv m3d: the up-conv's FORWARD on the f16 matrix cores at fp32 accuracy (m3d.compat.set_upconv_f16, "
                         "csrc/upconv3d_f16.hip); the backward follows --upconv-backward")
    ap.add_argument("--upconv-backward", choices=("fp32", "f16x2"), default="fp32",
                    help="with --upconv m3d: the up-conv's BACKWARD (m3d.compat.set_upconv_backward): f16x2 = csrc/upconv3d_bwd_f16.hip for "
                         "the directions conv_plan.upconv_backward_kernel routes to it")
    ap.add_argument("--mask-dilation", type=int, choices=(1, 2), default=1,
                    help="with --mask: MRCNN.DILATION of the mask head's 3^3 convs (MaskTrainCfg.dilation)")
    ap.add_argument("--conv-dilated", choices=("torch", "m3d"), default="torch",
                    help="the dilation-2 convs (m3d.compat.set_conv_dilated): m3d = the library's dilated forward, dgrad and wgrad "
                         "(csrc/conv3d_wgrad.hip)")
    ap.add_argument("--conv-dilated-f16", action="store_true",
                    help="with --conv-dilated m3d: forward and dgrad of the dilation-2 convs on maps at most 8 wide on the f16 matrix cores at "
                         "fp32 accuracy (m3d.compat.set_conv_dilated_f16)")
    ap.add_argument("--box-head", choices=("mlp", "conv"), default="mlp",
                    help="mlp = RoIAlign -> two FC layers (roi_2mlp_head); conv = m3d.ConvBoxHead (roi_Xconv1fc_head)")
    ap.add_argument("--conv-head-dim", type=int, default=128, help="with --box-head conv: FAST_RCNN.CONV_HEAD_DIM (the nuclei YAML has 128)")
    ap.add_argument("--conv-head-convs", type=int, default=2, help="with --box-head conv: FAST_RCNN.NUM_STACKED_CONVS (the nuclei YAML has 2)")
    ap.add_argument("--conv-narrow", choices=("fp32", "f16x2"), default="fp32",
                    help="forward and dgrad of the dilation-1 3^3 convs on maps at most 8 wide (the per-RoI convs): f16x2 = the narrow-map "
                         "kernel on the f16 matrix cores at fp32 accuracy (m3d.compat.set_conv_train_narrow)")
    ap.add_argument("--wgrad-narrow", action="store_true",
                    help="dilation-1 conv weight gradients on maps at most 8 wide (the per-RoI convs) on the 2 x 8 x 8 tile kernel "
                         "(m3d.compat.set_conv_wgrad_narrow)")
    ap.add_argument("--wgrad-narrow-f16", action="store_true",
                    help="weight gradients of those convs (cin and cout multiples of 32) on the f16 matrix cores at fp32 accuracy on the "
                         "2 x 8 x 8 tile (m3d.compat.set_conv_wgrad_narrow_f16)")
    ap.add_argument("--wgrad-dilated-f16", action="store_true",
                    help="with --mask spot --mask-dilation 2 --conv-dilated m3d: weight gradients of the dilation-2 convs on maps at most 8 "
                         "wide (cin and cout multiples of 32) on the f16 matrix cores at fp32 accuracy (m3d.compat.set_conv_wgrad_dilated_f16)")
    ap.add_argument("--linear-backward", choices=("fp32", "f16x2"), default="fp32",
                    help="backward of the FC layers (m3d.compat.set_linear_backward): f16x2 = the f16 matrix cores at fp32 accuracy where "
                         "conv_plan.linear_backward_kernel routes a layer")
    a = ap.parse_args()
    if a.mask_dilation != 1 and not a.mask:
        ap.error("--mask-dilation needs --mask")
    if a.upconv_f16 and a.upconv != "m3d":
        ap.error("--upconv-f16 needs --upconv m3d")
    if a.upconv_backward != "fp32" and a.upconv != "m3d":
        ap.error("--upconv-backward f16x2 needs --upconv m3d")
    if a.conv_dilated_f16 and a.conv_dilated != "m3d":
        ap.error("--conv-dilated-f16 needs --conv-dilated m3d")
    if a.wgrad_dilated_f16 and not (a.mask == "spot" and a.mask_dilation == 2 and a.conv_dilated == "m3d"):
        ap.error("--wgrad-dilated-f16 needs --mask spot --mask-dilation 2 --conv-dilated m3d")
    import torch
    import m3d
    import m3d.compat
    from m3d.synth import synth_volume, synth_volume_boxes
    from train_rpn import build_model
    assert torch.cuda.is_available(), "train_detector needs a GPU"
    m3d.compat.install()
    m3d.compat.set_conv_wgrad(a.wgrad)
    m3d.compat.set_conv_wgrad_narrow(a.wgrad_narrow)
    m3d.compat.set_conv_wgrad_narrow_f16(a.wgrad_narrow_f16)
    m3d.compat.set_conv_train_narrow(a.conv_narrow == "f16x2")
    m3d.compat.set_conv_train(a.conv)
    m3d.compat.set_roi_align_backward(a.roi_backward)
    m3d.compat.set_upconv(a.upconv)
    m3d.compat.set_upconv_f16(a.upconv_f16)
    m3d.compat.set_upconv_backward(a.upconv_backward)
    m3d.compat.set_conv_dilated(a.conv_dilated)
    m3d.compat.set_conv_dilated_f16(a.conv_dilated_f16)
    m3d.compat.set_conv_wgrad_dilated_f16(a.wgrad_dilated_f16)
    m3d.compat.set_linear_backward(a.linear_backward)
    torch.manual_seed(a.seed)
    tile = tuple(a.tile)
    rcfg, bcfg = m3d.RpnTrainCfg.nuclei(max_size=max(tile)), m3d.BoxHeadTrainCfg.nuclei()
    vol = synth_volume(0, tile).astype(np.float32)
    x = torch.from_numpy((vol - vol.mean()) / vol.std())[None, None].cuda()
    gt = torch.from_numpy(synth_volume_boxes(0, tile)).cuda()
    net = build_model(rcfg.num_anchors, a.width).cuda()
    if a.box_head == "conv":
        head = m3d.ConvBoxHead(8 * a.width, rcfg.stride, num_classes=bcfg.num_classes, conv_head_dim=a.conv_head_dim,
                               num_stacked_convs=a.conv_head_convs, mlp_head_dim=a.hidden).cuda()
    else:
        head = build_box_head(8 * a.width, a.hidden, bcfg.num_classes, rcfg.stride).cuda()
    net.train()
    for m in net.modules():                       # running statistics; the reference trains on batch statistics (m3d.train.DsnBody does)
        if isinstance(m, torch.nn.BatchNorm3d):
            m.eval()
    params = list(net.parameters()) + list(head.parameters())
    if a.mask:
        mcfg = m3d.MaskTrainCfg.soma(in_size=tile, dim_reduced=4 * a.width, num_convs=2, dilation=a.mask_dilation)
        mask_head = m3d.MaskHead(8 * a.width, mcfg, rcfg.stride).cuda()
        g = gt.cpu().numpy()                                                       # (x, y, z, r): centre and half the shortest edge
        spots = torch.from_numpy(np.concatenate([(g[:, :3] + g[:, 3:]) / 2, (g[:, 3:] - g[:, :3]).min(1, keepdims=True) / 2], 1)).cuda()
        params += list(mask_head.parameters())
    opt = torch.optim.SGD(params, lr=a.lr, momentum=0.9)
    im_info = np.array([tile[0], tile[1], tile[2], 1.0])
    for step in range(a.steps):
        seed = 1000 * a.seed + step                                                # one sampling seed per step
        feat = net.body(x)
        logits, pred = net.head(feat)
        loss_rpn_cls, loss_rpn_bbox = m3d.rpn_losses(logits, pred, m3d.rpn_targets(gt, tile, rcfg, seed=seed))
        with torch.no_grad():                                                      # generate_proposals_3d.py: no gradient through the proposals
            rois, _, _, num = m3d.generate_proposals3d_batched(torch.sigmoid(logits), pred, rcfg.cell_anchors, float(rcfg.stride), im_info,
                                                               1000, 2000, 0.7)
        targets = m3d.box_head_targets(rois, num, [gt], bcfg, seed=seed)
        cls_score, bbox_pred = head(feat, targets.rois7)
        loss_cls, loss_bbox, accuracy = m3d.box_head_losses(cls_score, bbox_pred, targets)
        total = loss_rpn_cls + loss_rpn_bbox + loss_cls + loss_bbox
        extra = ""
        if a.mask:
            mask_targets = m3d.mask_targets(targets, mcfg, spots=[spots])
            loss_mask = m3d.mask_losses(mask_head(feat, mask_targets.rois7), mask_targets)
            total = total + loss_mask
            extra = " loss_mask %.6f" % loss_mask.item()
        opt.zero_grad()
        total.backward()
        opt.step()
        print("step %d loss_rpn_cls %.6f loss_rpn_bbox %.6f loss_cls %.6f loss_bbox %.6f accuracy_cls %.4f%s total %.6f" % (
            step, loss_rpn_cls.item(), loss_rpn_bbox.item(), loss_cls.item(), loss_bbox.item(), accuracy.item(), extra, total.item()), flush=True)


if __name__ == "__main__":
    main()
