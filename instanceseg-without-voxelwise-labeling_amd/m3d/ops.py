"""Tensor-level wrappers over the C ABI (include/m3d.h).  Every function takes/returns torch CUDA tensors and
launches on the current torch stream; none of them synchronises unless the result size is data dependent."""
import ctypes as C
import math
import threading

import numpy as np
import torch

from ._lib import lib, check, M3DError, SgdTensor, AdamTensor, GradTensor, BoxHead, TrainImage, MaskImage

BBOX_XFORM_CLIP = float(np.log(1000. / 16.))   # lib/core/config.py:947

__all__ = ["compact_rows", "compact_rows2", "box_head_outputs", "roi_align3d_forward", "roi_align3d_backward", "roi_align3d_backward_ordered", "nms3d", "bbox_overlaps3d", "bbox_transform3d",
           "generate_proposals3d", "generate_proposals3d_batched", "box_results3d_batched", "nms3d_batched", "fused_max_boxes", "PackedConv3d", "maxpool3d_2x", "maxpool3d_2x_backward", "reduce_min", "reduce_min_multi", "norm1", "norm1_batched", "norm1_stats", "train_sample", "linear", "linear_plan", "linear_dgrad", "linear_wgrad", "linear_dgrad_f16x2", "linear_wgrad_f16x2", "linear_backward_f16x2_supported", "linear_dgrad_f16x2_plan", "linear_wgrad_f16x2_plan", "upconv3d_2x_forward", "upconv3d_2x_dgrad", "upconv3d_2x_wgrad", "upconv3d_2x_slices", "UPCONV_KINDS", "UpConvF16", "upconv3d_2x_dgrad_f16x2", "upconv3d_2x_wgrad_f16x2", "upconv3d_2x_backward_f16x2_supported", "upconv3d_2x_backward_f16x2_plan", "SplitLinear", "linear_roi_fused", "mask_paste3d",
           "otsu2d_batch", "prm_quantize_u8", "prm_quantize_windows_u8", "prm_quantize_windows_compact_u8", "roi_normalize", "conv3d_wgrad", "conv3d_wgrad_f16x2", "conv3d_wgrad_f16x2_supported", "conv3d_wgrad_f16x2_plan", "conv3d_wgrad_narrow_f16x2", "conv3d_wgrad_narrow_f16x2_supported", "conv3d_wgrad_narrow_f16x2_plan", "conv3d_direct_plan", "conv3d_bias_grad", "conv3d_gy_reduce", "WinoConv3d", "ZwConv3d", "ZnConv3d", "X3Conv3d", "StemWinoConv3d", "gaussian_filter_u16", "median_filter3_u16", "cc_largest_batch", "binary_closing6_batch", "paint_instances", "paint_instances_into", "paint_finish", "paint_begin", "crop_offsets", "upload_packed", "conv3d_windowed", "prm_seed", "strip_geometry", "prm_prepare_plan", "prm_stem_dgrad_plan", "PRM_PREPARE_KERNELS", "PRM_STEM_DGRAD_LAYOUTS", "prm_select_peaks", "PinnedPool", "upload", "prm_prepare", "prm_stem_dgrad", "prm_stem_prepare_weights", "SmallWindowDgrad", "prm_den_pool", "prm_stem_mfma_weights", "prm_stem_dgrad_fused", "prm_stem_dgrad_fused_supported", "prm_scatter", "conv3d_stem5_dgrad", "conv3d_stem5_dgrad_weights", "label_overlap", "label_iou_best", "box_union_overlap_counts", "Overlap", "IouBest", "LABEL_LIMIT", "label_components", "label_counts", "paint_spheres", "rpn_target_sets", "rpn_target_blobs", "rpn_loss_grad", "box_head_target_sets", "box_head_target_blobs", "box_head_loss_grad", "mask_target_sets", "mask_loss_grad", "bn_stats", "bn_invstd", "bn_apply", "bn_backward", "sgd_step", "sgd_chunk", "sgd_step_scaled", "adam_step", "grad_clip_coef", "M3DError", "BBOX_XFORM_CLIP", "W_PLAIN", "W_RELU", "W_DGRAD", "W_DGRAD_RELU"]

W_PLAIN, W_RELU, W_DGRAD, W_DGRAD_RELU = 0, 1, 2, 3


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_gpu(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise M3DError("m3d ops need CUDA (ROCm) tensors; there is no CPU path")


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _f32c(t):
    return t.contiguous().float() if (t.dtype != torch.float32 or not t.is_contiguous()) else t


def _claim(out):
    """A caller's `out=` tensor is about to be rewritten through ctypes, which does not bump its `_version`: drop the operand bounds an
    earlier launch left on it (`_m3d_bound`, `_m3d_peak_max`, also on the tensor it is a view of), or the next f16x2 conv would scale the
    new values by the old bound.  A launch that leaves a fresh bound sets it after this.  Other views of the same storage (siblings of
    `out`, or views of `out`) keep theirs: no caller leaves a bound on such a view, and one that did would have to drop it itself."""
    for t in (out, getattr(out, "_base", None)):
        if t is not None:
            t.__dict__.pop("_m3d_bound", None)
            t.__dict__.pop("_m3d_peak_max", None)


# ------------------------------------------------------------------ RoIAlign3D
def roi_align3d_forward(features, rois, AS, AH, AW, spatial_scale, sampling_ratio, exact=False, ordered=True, feat_absmax=None):
    """exact=True: the reference kernel's fp32 operation order (bit-identical to the oracle); default: the
    separable fast form (same samples and weights, different summation order).  ordered=False: RoIs launched in index order (A/B).
    feat_absmax (round 6; device floats whose largest is >= max |features|: ops.absmax, or the slot array the producing conv left): RoIs
    with sub-volumes of <= 128 voxels run as one GEMM per RoI on the f16 matrix cores (m3d_roi_align3d_forward_ws3); None keeps every RoI
    on the separable kernels."""
    _need_gpu(features, rois)
    features, rois = _f32c(features), _f32c(rois)
    B, Cc, S, H, W = features.shape
    R = rois.shape[0]
    # functions/roi_align_3d.py:24 zero-fills before the call; every forward kernel here writes every output element
    # (RoIs without a valid sample included), so the 351 MB memset is not repeated
    out = torch.empty((R, Cc, AS, AH, AW), dtype=torch.float32, device=features.device)
    cols = int(rois.shape[1]) if rois.dim() == 2 else 0
    if exact:
        check(lib().m3d_roi_align3d_forward_exact(int(AS), int(AH), int(AW), C.c_float(spatial_scale), int(sampling_ratio), _ptr(features), B, Cc, S, H, W,
                                                  _ptr(rois), R, cols, _ptr(out), _stream()), "roi_align3d_forward_exact")
        return out
    wsb = int(lib().m3d_roi_align3d_workspace_bytes(R)) if ordered else 0          # launch order (heaviest RoI first) + per-RoI set-up records
    ws = torch.empty((max(wsb, 4),), dtype=torch.uint8, device=features.device) if ordered else None
    if feat_absmax is not None and ordered:
        _need_gpu(feat_absmax)
        check(lib().m3d_roi_align3d_forward_ws3(int(AS), int(AH), int(AW), C.c_float(spatial_scale), int(sampling_ratio), _ptr(features), B, Cc, S, H, W,
                                                _ptr(rois), R, cols, _ptr(out), _ptr(ws), C.c_size_t(wsb), _ptr(feat_absmax),
                                                int(feat_absmax.numel()), _stream()), "roi_align3d_forward")
        return out
    check(lib().m3d_roi_align3d_forward_ws(int(AS), int(AH), int(AW), C.c_float(spatial_scale), int(sampling_ratio), _ptr(features), B, Cc, S, H, W,
                                           _ptr(rois), R, cols, _ptr(out), _ptr(ws), C.c_size_t(wsb), _stream()), "roi_align3d_forward")
    return out


def roi_align3d_backward(top_grad, rois, feature_size, AS, AH, AW, spatial_scale, sampling_ratio):
    _need_gpu(top_grad, rois)
    top_grad, rois = _f32c(top_grad), _f32c(rois)
    B, Cc, S, H, W = feature_size
    grad = torch.zeros((B, Cc, S, H, W), dtype=torch.float32, device=top_grad.device)      # roi_align_3d.py:41-42
    check(lib().m3d_roi_align3d_backward(int(AS), int(AH), int(AW), C.c_float(spatial_scale), int(sampling_ratio),
                                         _ptr(top_grad), _ptr(rois), rois.shape[0], int(rois.shape[1]), _ptr(grad),
                                         B, Cc, S, H, W, _stream()), "roi_align3d_backward")
    return grad


def roi_align3d_backward_ordered(top_grad, rois, feature_size, AS, AH, AW, spatial_scale, sampling_ratio):
    """roi_align3d_backward in gather form (m3d_roi_align3d_backward_ordered; DESIGN, "RoIAlign3D backward, ordered"): no atomics, the
    result bit-identical from call to call, every element written by the kernel (no zero fill).  Same arguments and return.  With a fixed
    sampling_ratio nothing is read back and the call can be captured into a graph; with an adaptive one (sampling_ratio <= 0) the status
    word is read - a synchronisation - and a RoI whose grid is beyond the tables raises M3DError: there is no fall-back to the atomic
    kernel."""
    _need_gpu(top_grad, rois)
    top_grad, rois = _f32c(top_grad), _f32c(rois)
    B, Cc, S, H, W = feature_size
    R = rois.shape[0]
    grad = torch.empty((B, Cc, S, H, W), dtype=torch.float32, device=top_grad.device)
    wsb = int(lib().m3d_roi_align3d_backward_ordered_workspace_bytes(R, B))
    ws = torch.empty((max(wsb, 4) + 3) // 4, dtype=torch.int32, device=top_grad.device)
    cols = int(rois.shape[1]) if rois.dim() == 2 else 0
    check(lib().m3d_roi_align3d_backward_ordered(int(AS), int(AH), int(AW), C.c_float(spatial_scale), int(sampling_ratio),
                                                 _ptr(top_grad), _ptr(rois), R, cols, _ptr(grad), B, Cc, S, H, W,
                                                 _ptr(ws), C.c_size_t(wsb), _stream()), "roi_align3d_backward_ordered")
    if int(sampling_ratio) <= 0 and int(ws[0]) != 0:
        raise M3DError("roi_align3d_backward_ordered: an adaptive sampling grid needs more than 64 table entries on an axis of some RoI "
                       "(bins * ceil(roi / bins) > 64); the ordered backward does not take it - nothing was written")
    return grad


# ------------------------------------------------------------------ NMS / IoU / decode
def nms3d(dets, thresh, by_volume=False):
    """dets [N,7] fp32 CUDA -> int64 CUDA tensor of kept input indices (ascending)."""
    _need_gpu(dets)
    dets = _f32c(dets)
    n = dets.shape[0]
    if n == 0:
        return torch.zeros((0,), dtype=torch.int64, device=dets.device)
    if dets.dim() != 2 or dets.shape[1] != 7:
        raise ValueError("dets must be [N,7]")
    if n <= fused_max_boxes():                       # the fused kernels (three launches instead of seven)
        # the count lands in pinned host memory, written by the kernel itself: a stream synchronize instead of a D2H copy
        # (N = 1000: 90 -> 78 us wall; the kernels themselves take 63 us back to back)
        dev = dets.device
        keep = torch.empty((1, n), dtype=torch.int64, device=dev)
        num = _pinned_i32(dev)
        wsb = lib().m3d_nms3d_batched_workspace_bytes(1)
        ws = _workspace(wsb, dev, "nmsb")
        check(lib().m3d_nms3d_batched(_ptr(dets), C.c_size_t(7 * n), None, 0, 1, n, C.c_float(np.float32(thresh)), int(bool(by_volume)),
                                      0, None, _ptr(keep), _ptr(num), _ptr(ws), C.c_size_t(wsb), _stream()), "nms3d_batched")
        torch.cuda.current_stream().synchronize()
        return keep[0, :int(num[0])]
    keep = torch.empty((n,), dtype=torch.int64, device=dets.device)
    num = torch.zeros((1,), dtype=torch.int32, device=dets.device)
    wsb = lib().m3d_nms3d_workspace_bytes(n)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dets.device)
    check(lib().m3d_nms3d(_ptr(dets), n, C.c_float(np.float32(thresh)), int(bool(by_volume)), _ptr(keep), _ptr(num),
                          _ptr(ws), C.c_size_t(wsb), _stream()), "nms3d")
    return keep[:int(num.item())]


def bbox_overlaps3d(boxes, query):
    _need_gpu(boxes, query)
    boxes, query = _f32c(boxes), _f32c(query)
    out = torch.empty((boxes.shape[0], query.shape[0]), dtype=torch.float32, device=boxes.device)
    check(lib().m3d_bbox_overlaps3d(_ptr(boxes), boxes.shape[0], _ptr(query), query.shape[0], _ptr(out), _stream()),
          "bbox_overlaps3d")
    return out


def bbox_transform3d(boxes, deltas, weights=(1.,) * 6, clip_to=None, xform_clip=BBOX_XFORM_CLIP):
    """boxes [N,6], deltas [N,6k] -> [N,6k]; clip_to=(slices,height,width) fuses clip_tiled_boxes_3d."""
    _need_gpu(boxes, deltas)
    boxes, deltas = _f32c(boxes), _f32c(deltas)
    n, k = boxes.shape[0], deltas.shape[1] // 6
    out = torch.empty_like(deltas)
    w = (C.c_double * 6)(*[float(x) for x in weights])
    cs, ch, cw = (0., 0., 0.) if clip_to is None else [float(v) for v in clip_to]
    check(lib().m3d_bbox_transform3d(_ptr(boxes), _ptr(deltas), n, k, w, C.c_double(xform_clip), C.c_double(cs),
                                     C.c_double(ch), C.c_double(cw), _ptr(out), _stream()), "bbox_transform3d")
    return out


def generate_proposals3d(scores, deltas, anchors, feat_stride, im_info, pre_nms_topN, post_nms_topN, nms_thresh,
                         min_size=0.0, batch_index=0, xform_clip=BBOX_XFORM_CLIP):
    """scores [A,S,H,W], deltas [6A,S,H,W] CUDA fp32; anchors [A,6] float64 numpy.
    Returns (rois [R,7] f32, probs [R,1] f32, keep_idx [R] i64) on device."""
    _need_gpu(scores, deltas)
    scores, deltas = _f32c(scores), _f32c(deltas)
    A, S, H, W = scores.shape
    assert deltas.shape == (6 * A, S, H, W)
    total = A * S * H * W
    K = total if (pre_nms_topN <= 0 or pre_nms_topN >= total) else pre_nms_topN
    cap = K
    dev = scores.device
    rois = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    probs = torch.empty((cap,), dtype=torch.float32, device=dev)
    kidx = torch.empty((cap,), dtype=torch.int64, device=dev)
    num = torch.zeros((1,), dtype=torch.int32, device=dev)
    wsb = lib().m3d_generate_proposals3d_workspace_bytes(A, S, H, W, int(pre_nms_topN))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    anc = np.ascontiguousarray(anchors, dtype=np.float64)
    info = np.ascontiguousarray(im_info, dtype=np.float64)
    check(lib().m3d_generate_proposals3d(_ptr(scores), _ptr(deltas), A, S, H, W, anc.ctypes.data_as(C.c_void_p),
                                         C.c_double(feat_stride), info.ctypes.data_as(C.c_void_p), int(pre_nms_topN),
                                         int(post_nms_topN), C.c_float(np.float32(nms_thresh)), C.c_double(min_size),
                                         C.c_double(xform_clip), int(batch_index), _ptr(rois), _ptr(probs), _ptr(kidx),
                                         _ptr(num), _ptr(ws), C.c_size_t(wsb), _stream()), "generate_proposals3d")
    r = int(num.item())
    return rois[:r], probs[:r].unsqueeze(1), kidx[:r]


# ------------------------------------------------------------------ batched, fused box stages (csrc/box_fused.hip)
def fused_max_boxes():
    return int(lib().m3d_fused_max_boxes())


_ws_cache = {}


_pin_cache = {}


def _pinned_i32(device):
    """One pinned int32 per device: a kernel writes a count there, the caller synchronizes its stream and reads it at once."""
    t = _pin_cache.get(str(device))
    if t is None:
        t = _pin_cache[str(device)] = torch.zeros((1,), dtype=torch.int32).pin_memory()
    return t


def _workspace(nbytes, device, tag):
    """One scratch buffer per (stream, stage): the fused stages are launched back to back on a stream, so re-using the
    buffer is safe, and allocating ~1 MB per tile on every call would cost more than the kernels."""
    key = (tag, torch.cuda.current_stream().cuda_stream, str(device))
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _ws_cache[key] = torch.empty((int(nbytes),), dtype=torch.uint8, device=device)
    return ws


def generate_proposals3d_batched(scores, deltas, anchors, feat_stride, im_info, pre_nms_topN, post_nms_topN, nms_thresh,
                                 min_size=0.0, first_batch_index=0, xform_clip=BBOX_XFORM_CLIP):
    """scores [B,A,S,H,W], deltas [B,6A,S,H,W] -> (rois [B,rows,7], probs [B,rows], keep_idx [B,rows], num int32 [B]), all on
    the device, ONE launch, no host synchronisation; item b's valid rows are [0, num[b])."""
    _need_gpu(scores, deltas)
    scores, deltas = _f32c(scores), _f32c(deltas)
    B, A, S, H, W = scores.shape
    assert deltas.shape == (B, 6 * A, S, H, W)
    total = A * S * H * W
    K = total if (pre_nms_topN <= 0 or pre_nms_topN >= total) else pre_nms_topN
    # post_nms_topN only cuts the list when NMS runs (generate_proposals_3d.py:167-171)
    rows = K if (post_nms_topN <= 0 or nms_thresh <= 0) else min(K, post_nms_topN)
    dev = scores.device
    rois = torch.empty((B, rows, 7), dtype=torch.float32, device=dev)
    probs = torch.empty((B, rows), dtype=torch.float32, device=dev)
    kidx = torch.empty((B, rows), dtype=torch.int64, device=dev)
    num = torch.empty((B,), dtype=torch.int32, device=dev)
    wsb = lib().m3d_generate_proposals3d_batched_workspace_bytes(B, A, S, H, W, int(pre_nms_topN))
    ws = _workspace(wsb, dev, "prop")
    anc = np.ascontiguousarray(anchors, dtype=np.float64)
    info = np.ascontiguousarray(im_info, dtype=np.float64)
    check(lib().m3d_generate_proposals3d_batched(_ptr(scores), _ptr(deltas), B, A, S, H, W, anc.ctypes.data_as(C.c_void_p),
                                                 C.c_double(feat_stride), info.ctypes.data_as(C.c_void_p), int(pre_nms_topN),
                                                 int(post_nms_topN), C.c_float(np.float32(nms_thresh)), C.c_double(min_size),
                                                 C.c_double(xform_clip), int(first_batch_index), rows, _ptr(rois), _ptr(probs),
                                                 _ptr(kidx), _ptr(num), _ptr(ws), C.c_size_t(wsb), _stream()),
          "generate_proposals3d_batched")
    return rois, probs, kidx, num


def compact_rows(src, counts, offsets=None):
    """src [B,rows,...] (contiguous, 4-byte elements or int64), counts int32 [B] on the device -> (packed [B*rows,...] whose first
    sum(counts) rows are item 0's valid rows, item 1's, ..., offsets int32 [B+1] on the device).  No host synchronisation: the caller
    slices `packed[:total]` once it knows the total."""
    _need_gpu(src, counts)
    assert src.is_contiguous() and counts.dtype == torch.int32 and counts.is_contiguous() and src.dim() >= 2
    B, rows = src.shape[0], src.shape[1]
    row_bytes = src[0, 0].numel() * src.element_size()
    out = torch.empty((B * rows,) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    if offsets is None:
        offsets = torch.empty((B + 1,), dtype=torch.int32, device=src.device)
    check(lib().m3d_compact_rows(_ptr(src), C.c_size_t(rows * row_bytes), C.c_size_t(row_bytes), _ptr(counts), B, rows, _ptr(out),
                                 _ptr(offsets), _stream()), "compact_rows")
    return out, offsets


def compact_rows2(src_a, src_b, counts, host_counts=None):
    """compact_rows of two row sets with the same counts in ONE launch -> (packed_a, packed_b, offsets int32 [B+1]).  host_counts: a
    PINNED int32 tensor [B] the kernel itself fills with the counts - record an event behind this call and wait for that."""
    _need_gpu(src_a, src_b, counts)
    assert src_a.is_contiguous() and src_b.is_contiguous() and counts.dtype == torch.int32 and counts.is_contiguous()
    B, rows = src_a.shape[0], src_a.shape[1]
    assert src_b.shape[0] == B and src_b.shape[1] == rows
    rb_a = src_a[0, 0].numel() * src_a.element_size()
    rb_b = src_b[0, 0].numel() * src_b.element_size()
    out_a = torch.empty((B * rows,) + tuple(src_a.shape[2:]), dtype=src_a.dtype, device=src_a.device)
    out_b = torch.empty((B * rows,) + tuple(src_b.shape[2:]), dtype=src_b.dtype, device=src_b.device)
    offsets = torch.empty((B + 1,), dtype=torch.int32, device=src_a.device)
    if host_counts is not None:
        assert host_counts.is_pinned() and host_counts.dtype == torch.int32 and host_counts.numel() >= B
    check(lib().m3d_compact_rows2(_ptr(src_a), C.c_size_t(rows * rb_a), C.c_size_t(rb_a), _ptr(src_b), C.c_size_t(rows * rb_b), C.c_size_t(rb_b),
                                  _ptr(counts), B, rows, _ptr(out_a), _ptr(out_b), _ptr(offsets),
                                  C.c_void_p(host_counts.data_ptr()) if host_counts is not None else None, _stream()), "compact_rows2")
    return out_a, out_b, offsets


def box_head_outputs(outs, rois, num_classes, weights, clip_to=None, xform_clip=BBOX_XFORM_CLIP):
    """outs [M, nc + 6 nc] (cls_score and bbox_pred as one GEMM), rois [M,7] -> (cls [M,nc] softmax, bbox [M,6nc] raw deltas,
    pred [M,6nc] decoded (+ clipped to clip_to = (slices, height, width))); one launch (m3d_box_head_outputs)."""
    _need_gpu(outs, rois)
    outs, rois = _f32c(outs), _f32c(rois)
    M, nc = int(outs.shape[0]), int(num_classes)
    assert outs.shape[1] == 7 * nc and rois.shape == (M, 7)
    cls = torch.empty((M, nc), dtype=torch.float32, device=outs.device)
    bbox = torch.empty((M, 6 * nc), dtype=torch.float32, device=outs.device)
    pred = torch.empty((M, 6 * nc), dtype=torch.float32, device=outs.device)
    w = (C.c_double * 6)(*[float(x) for x in weights])
    cs, ch, cw = (0., 0., 0.) if clip_to is None else [float(v) for v in clip_to]
    check(lib().m3d_box_head_outputs(_ptr(outs), _ptr(rois), M, nc, w, C.c_double(xform_clip), C.c_double(cs), C.c_double(ch), C.c_double(cw),
                                     _ptr(cls), _ptr(bbox), _ptr(pred), _stream()), "box_head_outputs")
    return cls, bbox, pred


def box_results3d_batched(scores, boxes, keep_idx, offsets, num_classes, score_thresh, nms_thresh, detections_per_im, max_rows):
    """scores [R,nc], boxes [R,6nc], keep_idx int64 [R] or None, offsets int32 [B+1] (device) ->
    (cls_boxes [B,nc,max_rows,7], cls_keep int64 [B,nc,max_rows], counts int32 [B,nc]); ONE launch, no host sync."""
    _need_gpu(scores, boxes, offsets)
    scores, boxes = _f32c(scores), _f32c(boxes)
    assert offsets.dtype == torch.int32 and offsets.is_contiguous()
    B = offsets.numel() - 1
    dev = scores.device
    cls_boxes = torch.empty((B, num_classes, max_rows, 7), dtype=torch.float32, device=dev)
    cls_keep = torch.empty((B, num_classes, max_rows), dtype=torch.int64, device=dev)
    counts = torch.empty((B, num_classes), dtype=torch.int32, device=dev)
    wsb = lib().m3d_box_results3d_batched_workspace_bytes(B)
    ws = _workspace(wsb, dev, "boxres")
    if keep_idx is not None:
        assert keep_idx.dtype == torch.int64 and keep_idx.is_contiguous()
    check(lib().m3d_box_results3d_batched(_ptr(scores), _ptr(boxes), _ptr(keep_idx), _ptr(offsets), B, int(num_classes),
                                          C.c_float(np.float32(score_thresh)), C.c_float(np.float32(nms_thresh)),
                                          int(detections_per_im), int(max_rows), _ptr(cls_boxes), _ptr(cls_keep), _ptr(counts),
                                          _ptr(ws), C.c_size_t(wsb), _stream()), "box_results3d_batched")
    return cls_boxes, cls_keep, counts


def nms3d_batched(dets, counts, thresh, by_volume=False, pack_cap=None, want_keep=True):
    """dets [B,n,7] (dim-0 stride arbitrary, inner dims contiguous), counts int32 view [B] (any stride) or None ->
    dict(keep int64 [B,n], num int32 [B], packed [B,pack_cap+1,7] if pack_cap is not None); ONE launch, no host sync."""
    _need_gpu(dets)
    assert dets.dim() == 3 and dets.shape[2] == 7 and dets.dtype == torch.float32 and dets.stride(2) == 1 and dets.stride(1) == 7
    B, n = dets.shape[0], dets.shape[1]
    dev = dets.device
    keep = torch.empty((B, n), dtype=torch.int64, device=dev) if want_keep else None
    num = torch.empty((B,), dtype=torch.int32, device=dev)
    packed = torch.empty((B, pack_cap + 1, 7), dtype=torch.float32, device=dev) if pack_cap is not None else None
    cstride = 0
    if counts is not None:
        assert counts.dtype == torch.int32 and counts.dim() == 1 and counts.numel() == B
        cstride = counts.stride(0)
    wsb = lib().m3d_nms3d_batched_workspace_bytes(B)
    ws = _workspace(wsb, dev, "nmsb")
    check(lib().m3d_nms3d_batched(_ptr(dets), C.c_size_t(dets.stride(0)), _ptr(counts), int(cstride), B, n,
                                  C.c_float(np.float32(thresh)), int(bool(by_volume)), int(pack_cap or 0), _ptr(packed), _ptr(keep),
                                  _ptr(num), _ptr(ws), C.c_size_t(wsb), _stream()), "nms3d_batched")
    return dict(keep=keep, num=num, packed=packed)


# ------------------------------------------------------------------ conv / pool
class PackedConv3d:
    """A Conv3d weight packed once into MFMA A-fragment order (m3d_conv3d_pack_weights)."""

    def __init__(self, weight, mode=W_PLAIN):
        _need_gpu(weight)
        weight = _f32c(weight)
        self.cout_w, self.cin_w, self.k = weight.shape[0], weight.shape[1], weight.shape[2]
        assert weight.shape[2] == weight.shape[3] == weight.shape[4]
        self.mode = mode
        dgrad = mode in (W_DGRAD, W_DGRAD_RELU)
        self.cin = self.cout_w if dgrad else self.cin_w      # logical conv this pack implements
        self.cout = self.cin_w if dgrad else self.cout_w
        nbytes = lib().m3d_conv3d_packed_weight_bytes(self.cin_w, self.cout_w, self.k, mode)
        self.packed = torch.empty((nbytes // 4,), dtype=torch.float32, device=weight.device)
        check(lib().m3d_conv3d_pack_weights(_ptr(weight), self.cin_w, self.cout_w, self.k, mode, _ptr(self.packed), _stream()),
              "conv3d_pack_weights")

    def supports_pool(self, width, voxels=None):
        """Fused conv+pool exists for the 5^3 stem and for k=3 on 32-wide x blocks; it uses the big 32x4x4 tile, so
        it only pays when that tile still yields >= 512 workgroups (same rule as the C dispatcher)."""
        if self.k == 5 and self.cin == 1 and self.cout <= 32:
            return True
        if self.k != 3 or width < 24:
            return False
        return voxels is None or (voxels // 512) * ((self.cout + 63) // 64) >= 512

    def pooled(self, x, scale=None, shift=None, relu=False, in_offset=None, return_argmax=False):
        """conv + scale/shift + ReLU + MaxPool3d(2,2) in one kernel (m3d_conv3d_forward_pool2)."""
        _need_gpu(x)
        x = _f32c(x)
        B, Cin, D, H, W = x.shape
        if Cin != self.cin:
            raise ValueError("expected %d input channels, got %d" % (self.cin, Cin))
        out = torch.empty((B, self.cout, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
        am = torch.empty(out.shape, dtype=torch.uint8, device=x.device) if return_argmax else None
        check(lib().m3d_conv3d_forward_pool2(_ptr(x), _ptr(self.packed), _ptr(out), _ptr(am), B, Cin, self.cout, D, H, W,
                                             self.k, _ptr(in_offset), _ptr(scale), _ptr(shift), int(bool(relu)), _stream()),
              "conv3d_forward_pool2")
        return (out, am) if return_argmax else out

    def split_sigmoid(self, x, split, shift=None):
        """One conv, two epilogues (m3d_conv3d_forward_split_sigmoid): (sigmoid(conv)[:, :split], conv[:, split:]) as two contiguous
        tensors - the RPN's cls_score + sigmoid and bbox_pred heads (rpn_heads.py:96-98,116)."""
        _need_gpu(x)
        x = _f32c(x)
        B, Cin, D, H, W = x.shape
        if Cin != self.cin:
            raise ValueError("expected %d input channels, got %d" % (self.cin, Cin))
        a = torch.empty((B, split, D, H, W), dtype=torch.float32, device=x.device)
        b = torch.empty((B, self.cout - split, D, H, W), dtype=torch.float32, device=x.device)
        check(lib().m3d_conv3d_forward_split_sigmoid(_ptr(x), _ptr(self.packed), _ptr(a), _ptr(b), B, Cin, self.cout, int(split), D, H, W, self.k,
                                                     _ptr(shift), _stream()), "conv3d_forward_split_sigmoid")
        return a, b

    def __call__(self, x, scale=None, shift=None, relu=False, in_offset=None, mul=None, out=None, dilation=1):
        _need_gpu(x)
        x = _f32c(x)
        B, Cin, D, H, W = x.shape
        if Cin != self.cin:
            raise ValueError("expected %d input channels, got %d" % (self.cin, Cin))
        _claim(out)
        if out is None:
            out = torch.empty((B, self.cout, D, H, W), dtype=torch.float32, device=x.device)
        for t in (scale, shift):
            if t is not None:
                assert t.is_cuda and t.dtype == torch.float32 and t.numel() == self.cout and t.is_contiguous()
        if dilation != 1:                                     # mask head (mask_rcnn_heads.py:148-151): padding = dilation
            assert in_offset is None and mul is None
            check(lib().m3d_conv3d_forward_dilated(_ptr(x), _ptr(self.packed), _ptr(out), B, Cin, self.cout, D, H, W, self.k,
                                                   int(dilation), _ptr(scale), _ptr(shift), int(bool(relu)), _stream()),
                  "conv3d_forward_dilated")
            return out
        if mul is not None:
            assert mul.shape == out.shape and mul.is_contiguous() and mul.dtype == torch.float32
        check(lib().m3d_conv3d_forward(_ptr(x), _ptr(self.packed), _ptr(out), B, Cin, self.cout, D, H, W, self.k,
                                       _ptr(in_offset), _ptr(scale), _ptr(shift), int(bool(relu)), _ptr(mul), _stream()),
              "conv3d_forward")
        return out


def conv3d_direct_plan(batch, cin, cout, depth, height, width, k=3, pool=False):
    """What PackedConv3d launches for this shape (m3d_conv3d_direct_plan, host only): a dict of the instantiation's dense id `variant`
    (below m3d_conv3d_direct_plan_count()), `cc` input channels per staged chunk, the voxel tile `tile_x`, `tile_y`, `tile_z`, `ncb` 32-channel
    output blocks per workgroup and `ksplit` - or None where the launch would return M3D_EUNSUPPORTED."""
    v = [C.c_int(-1) for _ in range(7)]
    rc = lib().m3d_conv3d_direct_plan(int(batch), int(cin), int(cout), int(depth), int(height), int(width), int(k), int(bool(pool)),
                                      *[C.byref(c) for c in v])
    if rc == -4:                                            # M3D_EUNSUPPORTED
        return None
    check(rc, "conv3d_direct_plan")
    return dict(zip(("variant", "cc", "tile_x", "tile_y", "tile_z", "ncb", "ksplit"), (c.value for c in v)))


class X3Conv3d:
    """A 3x3x3 'same' conv at fp32 accuracy on the bf16 matrix cores (csrc/conv3d_x3.hip: exact three-way bf16 cut of both operands,
    six products per fp32 product) - the exact direct kernel for the PRM norm convs: out = conv3d(x - in_offset, W or relu(W), padding 1).
    weight [cout, cin, 3, 3, 3]; mode W_PLAIN or W_RELU."""

    @staticmethod
    def supported(weight):
        return weight.dim() == 5 and tuple(weight.shape[2:]) == (3, 3, 3) and bool(lib().m3d_conv3d_x3_supported(weight.shape[1], weight.shape[0]))

    def __init__(self, weight, mode=W_PLAIN, f16=False):
        """f16 (round 6): the f16x2 split - two scaled fp16 pieces per operand, three products per fp32 product (m3d_conv3d_x3f_*); the call then
        needs `in_max` (a device scalar: max x with in_offset, max |x| without)."""
        _need_gpu(weight)
        weight = _f32c(weight)
        assert mode in (W_PLAIN, W_RELU) and X3Conv3d.supported(weight)
        self.cout, self.cin = weight.shape[0], weight.shape[1]
        self.f16 = bool(f16)
        if self.f16:
            nbytes = lib().m3d_conv3d_x3f_packed_bytes(self.cin, self.cout)
            self.packed = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
            check(lib().m3d_conv3d_x3f_pack(_ptr(weight), self.cin, self.cout, int(mode == W_RELU), _ptr(self.packed), _stream()), "conv3d_x3f_pack")
            return
        nbytes = lib().m3d_conv3d_x3_packed_bytes(self.cin, self.cout)
        self.packed = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
        check(lib().m3d_conv3d_x3_pack(_ptr(weight), self.cin, self.cout, int(mode == W_RELU), _ptr(self.packed), _stream()), "conv3d_x3_pack")

    def workgroups(self, shape):
        """launch size for x of `shape` [B, cin, D, H, W]: the library's own count (64 output channels x 16 x 4 x 4 voxels per
        workgroup, times the K ranges m3d_conv3d_x3_forward_ws cuts a small launch into)"""
        B, _, D, H, W = shape
        return int(lib().m3d_conv3d_x3_launch_units(int(B), self.cin, self.cout, int(D), int(H), int(W)))

    def __call__(self, x, in_offset=None, out=None, in_max=None):
        _need_gpu(x)
        x = _f32c(x)
        B, Cin, D, H, W = x.shape
        if Cin != self.cin:
            raise ValueError("expected %d input channels, got %d" % (self.cin, Cin))
        if self.f16 and in_max is None:
            raise ValueError("X3Conv3d(f16=True) needs in_max (ops.reduce_minmax_multi / ops.absmax)")
        _claim(out)
        if out is None:
            out = torch.empty((B, self.cout, D, H, W), dtype=torch.float32, device=x.device)
        wsb = lib().m3d_conv3d_x3_workspace_bytes(B, Cin, self.cout, D, H, W)
        ws = None
        if wsb:
            key = (torch.cuda.current_stream().cuda_stream, x.device)           # one scratch buffer per stream (the norm convs run on their own)
            cache = self.__dict__.setdefault("_ws", {})
            ws = cache.get(key)
            if ws is None or ws.numel() < wsb:
                ws = cache[key] = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
        if self.f16:
            _need_gpu(in_max)
            check(lib().m3d_conv3d_x3f_forward_ws(_ptr(x), _ptr(self.packed), _ptr(out), B, Cin, self.cout, D, H, W, _ptr(in_offset), _ptr(in_max),
                                                  _ptr(ws), C.c_size_t(wsb), _stream()), "conv3d_x3f_forward")
            return out
        check(lib().m3d_conv3d_x3_forward_ws(_ptr(x), _ptr(self.packed), _ptr(out), B, Cin, self.cout, D, H, W, _ptr(in_offset), _ptr(ws),
                                             C.c_size_t(wsb), _stream()), "conv3d_x3_forward")
        return out


def maxpool3d_2x(x, return_argmax=False):
    _need_gpu(x)
    x = _f32c(x)
    B, Cc, D, H, W = x.shape
    out = torch.empty((B, Cc, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
    am = torch.empty(out.shape, dtype=torch.uint8, device=x.device) if return_argmax else None
    check(lib().m3d_maxpool3d_2x_forward(_ptr(x), _ptr(out), _ptr(am), B * Cc, D, H, W, _stream()), "maxpool3d_2x_forward")
    return (out, am) if return_argmax else out


def maxpool3d_2x_backward(grad_out, argmax, in_shape):
    _need_gpu(grad_out, argmax)
    grad_out = _f32c(grad_out)
    B, Cc, D, H, W = in_shape
    gin = torch.empty(in_shape, dtype=torch.float32, device=grad_out.device)
    check(lib().m3d_maxpool3d_2x_backward(_ptr(grad_out), _ptr(argmax), _ptr(gin), B * Cc, D, H, W, _stream()),
          "maxpool3d_2x_backward")
    return gin


def reduce_min(x):
    _need_gpu(x)
    x = _f32c(x)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    wsb = lib().m3d_reduce_min_workspace_bytes()
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    check(lib().m3d_reduce_min(_ptr(x), C.c_int64(x.numel()), _ptr(out), _ptr(ws), C.c_size_t(wsb), _stream()), "reduce_min")
    return out


REDUCE_MIN_MULTI_MAX = 12      # kMinMulti of csrc/pool_bn.hip: m3d_reduce_min_multi returns M3D_EINVAL beyond it


def reduce_min_multi(xs):
    """Minima of any number of tensors, two launches per group of up to 12 (the entry point's capacity) -> float32 [len(xs)]
    (slice i:i+1 is the device scalar of tensor i)."""
    _need_gpu(*xs)
    xs = [_f32c(x) for x in xs]
    n = len(xs)
    out = torch.empty((max(n, 1),), dtype=torch.float32, device=xs[0].device)
    wsb = lib().m3d_reduce_min_multi_workspace_bytes()
    for g0 in range(0, n, REDUCE_MIN_MULTI_MAX):
        grp = xs[g0:g0 + REDUCE_MIN_MULTI_MAX]
        m = len(grp)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=xs[0].device)      # per group: the groups' launches are in flight together
        ptrs = (C.c_void_p * m)(*[x.data_ptr() for x in grp])
        cnts = (C.c_int64 * m)(*[x.numel() for x in grp])
        check(lib().m3d_reduce_min_multi(ptrs, cnts, m, _ptr(out[g0:g0 + m]), _ptr(ws), C.c_size_t(wsb), _stream()), "reduce_min_multi")
    return out


def reduce_minmax_multi(xs):
    """(minima, maxima) of any number of tensors, two launches per group of up to 12 -> two float32 [len(xs)] device tensors."""
    _need_gpu(*xs)
    xs = [_f32c(x) for x in xs]
    n = len(xs)
    out = torch.empty((2, max(n, 1)), dtype=torch.float32, device=xs[0].device)
    wsb = lib().m3d_reduce_minmax_multi_workspace_bytes()
    for g0 in range(0, n, REDUCE_MIN_MULTI_MAX):
        grp = xs[g0:g0 + REDUCE_MIN_MULTI_MAX]
        m = len(grp)
        ws = torch.empty((wsb,), dtype=torch.uint8, device=xs[0].device)
        ptrs = (C.c_void_p * m)(*[x.data_ptr() for x in grp])
        cnts = (C.c_int64 * m)(*[x.numel() for x in grp])
        check(lib().m3d_reduce_minmax_multi(ptrs, cnts, m, _ptr(out[0, g0:g0 + m]), _ptr(out[1, g0:g0 + m]), _ptr(ws), C.c_size_t(wsb), _stream()),
              "reduce_minmax_multi")
    return out[0], out[1]


def linear(x, weight, bias=None, relu=False, out=None):
    """act(x @ weight.T + bias) on the split-K fp32 MFMA GEMM (m3d_linear_forward): x [M,K], weight [N,K] (nn.Linear layout),
    bias [N] or None -> [M,N].  fast_rcnn_heads.py:84-85,114-115,15-19."""
    _need_gpu(x, weight, bias)
    x, weight = _f32c(x), _f32c(weight)
    M, K = x.shape
    N = weight.shape[0]
    if weight.shape[1] != K:
        raise ValueError("linear: x is [%d,%d] but weight is %s" % (M, K, tuple(weight.shape)))
    if bias is not None:
        bias = _f32c(bias)
        assert bias.numel() == N
    _claim(out)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=x.device)
    if M == 0:
        return out
    wsb = lib().m3d_linear_workspace_bytes(M, N, K)
    ws = torch.empty((max(wsb, 16) // 4,), dtype=torch.float32, device=x.device)
    check(lib().m3d_linear_forward(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), M, N, K, int(bool(relu)), _ptr(ws),
                                   C.c_size_t(wsb), _stream()), "linear_forward")
    return out


LINEAR_KINDS = ("fp32", "bf16x3", "bf16x3_w32", "f16x2")


def linear_plan(kind, M, N, K):
    """What the forward linear launch of `kind` (0 `linear`, 1 SplitLinear's packed kernels, 2 its "w32" kernel, 3 SplitLinearF16; or the
    name in LINEAR_KINDS) runs for x [M, K], weight [N, K] (m3d_linear_plan, host only): dict(tile_rows, tile_cols, slices, slices_tail,
    full_row_tiles) - the workgroup tile names the kernel instantiation; slices_tail / full_row_tiles: the fp32 kernel's ragged last row
    tile.  None where the launch would refuse the shape (K % 4, K % 32)."""
    if isinstance(kind, str):
        kind = LINEAR_KINDS.index(kind)
    v = [C.c_int(0) for _ in range(5)]
    rc = lib().m3d_linear_plan(int(kind), int(M), int(N), int(K), *[C.byref(a) for a in v])
    if rc == -4:
        return None
    check(rc, "linear_plan")
    return dict(zip(("tile_rows", "tile_cols", "slices", "slices_tail", "full_row_tiles"), (a.value for a in v)))


def linear_dgrad(gy, weight, out=None):
    """The input gradient of `linear`: gy [M,N] @ weight [N,K] -> [M,K] (m3d_linear_dgrad), on the weight as nn.Linear stores it - no
    transposed copy.  weight: K % 4 == 0, 16-byte aligned; gy: any M, N.  Autograd of fast_rcnn_heads.py:84-85,114-117,15-19,42-45."""
    _need_gpu(gy, weight)
    gy, weight = _f32c(gy), _f32c(weight)
    M, N = gy.shape
    K = weight.shape[1]
    if weight.shape[0] != N:
        raise ValueError("linear_dgrad: gy is [%d,%d] but weight is %s" % (M, N, tuple(weight.shape)))
    _claim(out)
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=gy.device)
    wsb = lib().m3d_linear_dgrad_workspace_bytes(M, N, K)
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=gy.device) if wsb else None
    check(lib().m3d_linear_dgrad(_ptr(gy), _ptr(weight), _ptr(out), M, N, K, _ptr(ws), C.c_size_t(wsb), _stream()), "linear_dgrad")
    return out


def linear_wgrad(gy, x, bias=True, out=None):
    """The weight and bias gradients of `linear` in one launch: (gy.T [N,M] @ x [M,K] -> [N,K], gy.sum(0) -> [N] or None without
    `bias`) (m3d_linear_wgrad), on both operands as they are - no transposed copy; an empty batch gives zeros.  x: K % 4 == 0, 16-byte
    aligned; gy: any M, N.  `out`: the [N,K] tensor to write.  Autograd of fast_rcnn_heads.py:84-85,114-117,15-19,42-45."""
    _need_gpu(gy, x)
    gy, x = _f32c(gy), _f32c(x)
    M, N = gy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError("linear_wgrad: gy is [%d,%d] but x is %s" % (M, N, tuple(x.shape)))
    _claim(out)
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=gy.device)
    gb = torch.empty((N,), dtype=torch.float32, device=gy.device) if bias else None
    wsb = lib().m3d_linear_wgrad_workspace_bytes(M, N, K)
    ws = torch.empty((wsb // 4,), dtype=torch.float32, device=gy.device) if wsb else None
    check(lib().m3d_linear_wgrad(_ptr(gy), _ptr(x), _ptr(out), _ptr(gb), M, N, K, _ptr(ws), C.c_size_t(wsb), _stream()), "linear_wgrad")
    return out, gb


def linear_backward_f16x2_supported(M, N, K):
    """m3d_linear_backward_f16x2_supported (host only): linear_dgrad_f16x2 / linear_wgrad_f16x2 take gy [M,N], weight [N,K], x [M,K]:
    M >= 1, N >= 64, N % 4 == 0, K % 4 == 0, no operand of 2^31 elements or more"""
    return bool(lib().m3d_linear_backward_f16x2_supported(int(M), int(N), int(K)))


def _linear_backward_f16x2_plan(fn, what, M, N, K):
    v = [C.c_int(0) for _ in range(3)]
    rc = fn(int(M), int(N), int(K), *[C.byref(a) for a in v])
    if rc == -4:
        return None
    check(rc, what)
    return dict(zip(("slices", "chain", "folds"), (a.value for a in v)))


def linear_dgrad_f16x2_plan(M, N, K):
    """What linear_dgrad_f16x2 runs for the shape (m3d_linear_dgrad_f16x2_plan, host only): dict(slices, chain, folds) - the slices of
    the reduction over N, the most MFMAs one accumulator chains (<= 384) and the folds of a slice's accumulator into fp32 registers;
    None where the shape is not supported."""
    return _linear_backward_f16x2_plan(lib().m3d_linear_dgrad_f16x2_plan, "linear_dgrad_f16x2_plan", M, N, K)


def linear_wgrad_f16x2_plan(M, N, K):
    """linear_dgrad_f16x2_plan for linear_wgrad_f16x2 (m3d_linear_wgrad_f16x2_plan): the reduction runs over M"""
    return _linear_backward_f16x2_plan(lib().m3d_linear_wgrad_f16x2_plan, "linear_wgrad_f16x2_plan", M, N, K)


def _bound_arg(what, b):
    """(pointer, slots) of an operand bound: None (the library sweeps), or 1 / ZwConv3d.SLOTS contiguous device floats (largest wins)"""
    if b is None:
        return _ptr(None), 0
    _need_gpu(b)
    if not (b.dtype == torch.float32 and b.is_contiguous() and b.numel() in (1, ZwConv3d.SLOTS)):
        raise ValueError("%s: a bound is 1 or %d contiguous float32 device values" % (what, ZwConv3d.SLOTS))
    return _ptr(b), int(b.numel())


def linear_dgrad_f16x2(gy, weight, gy_max=None, w_max=None, out=None):
    """linear_dgrad on the f16 matrix cores at fp32 accuracy (m3d_linear_dgrad_f16x2; csrc/fc_backward_f16.hip): gy [M,N] @ weight [N,K]
    -> [M,K], both operands read as fp32 and cut while they are staged - no pack, no transposed copy.  gy_max / w_max: device floats
    whose largest bounds |gy| / |weight| (ops.absmax, or a [ZwConv3d.SLOTS] array); None: the library sweeps that operand.  An
    unsupported shape is an error: ask linear_backward_f16x2_supported (or conv_plan.linear_backward_kernel)."""
    _need_gpu(gy, weight)
    gy, weight = _f32c(gy), _f32c(weight)
    M, N = gy.shape
    K = weight.shape[1]
    if weight.shape[0] != N:
        raise ValueError("linear_dgrad_f16x2: gy is [%d,%d] but weight is %s" % (M, N, tuple(weight.shape)))
    gp, gn = _bound_arg("linear_dgrad_f16x2", gy_max)
    wp, wn = _bound_arg("linear_dgrad_f16x2", w_max)
    _claim(out)
    if out is None:
        out = torch.empty((M, K), dtype=torch.float32, device=gy.device)
    wsb = lib().m3d_linear_dgrad_f16x2_workspace_bytes(M, N, K)
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=gy.device)
    check(lib().m3d_linear_dgrad_f16x2(_ptr(gy), _ptr(weight), _ptr(out), M, N, K, gp, gn, wp, wn, _ptr(ws), C.c_size_t(wsb), _stream()),
          "linear_dgrad_f16x2")
    return out


def linear_wgrad_f16x2(gy, x, gy_max=None, x_max=None, bias=True, out=None):
    """linear_wgrad on the f16 matrix cores at fp32 accuracy (m3d_linear_wgrad_f16x2): (gy.T @ x -> [N,K], gy.sum(0) -> [N] or None
    without `bias`); the bias gradient is summed from the uncut fp32 values.  Bounds as linear_dgrad_f16x2."""
    _need_gpu(gy, x)
    gy, x = _f32c(gy), _f32c(x)
    M, N = gy.shape
    K = x.shape[1]
    if x.shape[0] != M:
        raise ValueError("linear_wgrad_f16x2: gy is [%d,%d] but x is %s" % (M, N, tuple(x.shape)))
    gp, gn = _bound_arg("linear_wgrad_f16x2", gy_max)
    xp, xn = _bound_arg("linear_wgrad_f16x2", x_max)
    _claim(out)
    if out is None:
        out = torch.empty((N, K), dtype=torch.float32, device=gy.device)
    gb = torch.empty((N,), dtype=torch.float32, device=gy.device) if bias else None
    wsb = lib().m3d_linear_wgrad_f16x2_workspace_bytes(max(M, 1), N, K)
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=gy.device)
    check(lib().m3d_linear_wgrad_f16x2(_ptr(gy), _ptr(x), _ptr(out), _ptr(gb), M, N, K, gp, gn, xp, xn, _ptr(ws), C.c_size_t(wsb),
                                       _stream()), "linear_wgrad_f16x2")
    return out, gb


def _upconv_dims(what, weight, x=None, g=None):
    """(R, Cin, Cout, D, H, W) of an up-conv call from weight [Cin,Cout,2,2,2] and x [R,Cin,D,H,W] and / or g [R,Cout,2D,2H,2W]"""
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (2, 2, 2):
        raise ValueError("%s: weight must be [Cin, Cout, 2, 2, 2], got %s" % (what, tuple(weight.shape)))
    cin, cout = int(weight.shape[0]), int(weight.shape[1])
    if x is not None:
        if x.dim() != 5 or x.shape[1] != cin:
            raise ValueError("%s: x is %s but weight is %s" % (what, tuple(x.shape), tuple(weight.shape)))
        R, D, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), int(x.shape[4])
    else:
        if g.dim() != 5 or any(int(s) % 2 for s in g.shape[2:]):
            raise ValueError("%s: gy must be [R, Cout, 2D, 2H, 2W], got %s" % (what, tuple(g.shape)))
        R, D, H, W = int(g.shape[0]), int(g.shape[2]) // 2, int(g.shape[3]) // 2, int(g.shape[4]) // 2
    if g is not None and tuple(g.shape) != (R, cout, 2 * D, 2 * H, 2 * W):
        raise ValueError("%s: gy is %s, expected %s" % (what, tuple(g.shape), (R, cout, 2 * D, 2 * H, 2 * W)))
    return R, cin, cout, D, H, W


UPCONV_KINDS = ("forward", "dgrad", "wgrad")


def upconv3d_2x_slices(kind, R, Cin, Cout, D, H, W):
    """The partial sums an output element of the up-conv launch `kind` (a name in UPCONV_KINDS) is added up from at this shape
    (m3d_upconv3d_2x_slices, host only): 1 where the reduction is not split; 0 for a shape the launch refuses."""
    return int(lib().m3d_upconv3d_2x_slices(UPCONV_KINDS.index(kind), int(R), int(Cin), int(Cout), int(D), int(H), int(W)))


def upconv3d_2x_forward(x, weight, bias=None, relu=False, out=None):
    """ConvTranspose3d(kernel 2, stride 2, padding 0) with bias and ReLU in the epilogue (m3d_upconv3d_2x_forward): x [R,Cin,D,H,W],
    weight [Cin,Cout,2,2,2] as nn.ConvTranspose3d stores it, bias [Cout] or None -> [R,Cout,2D,2H,2W].  mask_rcnn_heads.py:156,193."""
    _need_gpu(x, weight, bias)
    x, weight = _f32c(x), _f32c(weight)
    R, cin, cout, D, H, W = _upconv_dims("upconv3d_2x_forward", weight, x=x)
    if bias is not None:
        bias = _f32c(bias)
        if bias.numel() != cout:
            raise ValueError("upconv3d_2x_forward: bias has %d elements, Cout is %d" % (bias.numel(), cout))
    _claim(out)
    if out is None:
        out = torch.empty((R, cout, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    check(lib().m3d_upconv3d_2x_forward(_ptr(x), _ptr(weight), _ptr(bias), _ptr(out), R, cin, cout, D, H, W, int(bool(relu)), _stream()),
          "upconv3d_2x_forward")
    return out


def upconv3d_2x_dgrad(gy, weight, y=None, out=None):
    """The input gradient of upconv3d_2x_forward (m3d_upconv3d_2x_dgrad): gy [R,Cout,2D,2H,2W], weight [Cin,Cout,2,2,2] -> [R,Cin,D,H,W].
    y: the output of a relu forward - gy counts only where y > 0, applied while gy is staged (None: no ReLU)."""
    _need_gpu(gy, weight, y)
    gy, weight = _f32c(gy), _f32c(weight)
    R, cin, cout, D, H, W = _upconv_dims("upconv3d_2x_dgrad", weight, g=gy)
    if y is not None:
        y = _f32c(y)
        if y.shape != gy.shape:
            raise ValueError("upconv3d_2x_dgrad: y is %s but gy is %s" % (tuple(y.shape), tuple(gy.shape)))
    _claim(out)
    if out is None:
        out = torch.empty((R, cin, D, H, W), dtype=torch.float32, device=gy.device)
    wsb = lib().m3d_upconv3d_2x_dgrad_workspace_bytes(R, cin, cout, D, H, W)
    ws = _workspace(wsb, gy.device, "upconv") if wsb else None
    check(lib().m3d_upconv3d_2x_dgrad(_ptr(gy), _ptr(y), _ptr(weight), _ptr(out), R, cin, cout, D, H, W, _ptr(ws), C.c_size_t(wsb),
                                      _stream()), "upconv3d_2x_dgrad")
    return out


def upconv3d_2x_wgrad(gy, x, y=None, bias=True, out=None):
    """The weight and bias gradients of upconv3d_2x_forward out of one launch (m3d_upconv3d_2x_wgrad): gy [R,Cout,2D,2H,2W], x
    [R,Cin,D,H,W] -> ([Cin,Cout,2,2,2], [Cout] or None without `bias`); an empty batch gives zeros.  y: as upconv3d_2x_dgrad."""
    _need_gpu(gy, x, y)
    gy, x = _f32c(gy), _f32c(x)
    if gy.dim() != 5 or x.dim() != 5:
        raise ValueError("upconv3d_2x_wgrad: gy is %s, x is %s" % (tuple(gy.shape), tuple(x.shape)))
    cin, cout = int(x.shape[1]), int(gy.shape[1])
    R, D, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), int(x.shape[4])
    if tuple(gy.shape) != (R, cout, 2 * D, 2 * H, 2 * W):
        raise ValueError("upconv3d_2x_wgrad: gy is %s, expected %s" % (tuple(gy.shape), (R, cout, 2 * D, 2 * H, 2 * W)))
    if y is not None:
        y = _f32c(y)
        if y.shape != gy.shape:
            raise ValueError("upconv3d_2x_wgrad: y is %s but gy is %s" % (tuple(y.shape), tuple(gy.shape)))
    _claim(out)
    if out is None:
        out = torch.empty((cin, cout, 2, 2, 2), dtype=torch.float32, device=gy.device)
    gb = torch.empty((cout,), dtype=torch.float32, device=gy.device) if bias else None
    wsb = lib().m3d_upconv3d_2x_wgrad_workspace_bytes(R, cin, cout, D, H, W)
    ws = _workspace(wsb, gy.device, "upconv") if wsb else None
    check(lib().m3d_upconv3d_2x_wgrad(_ptr(gy), _ptr(y), _ptr(x), _ptr(out), _ptr(gb), R, cin, cout, D, H, W, _ptr(ws), C.c_size_t(wsb),
                                      _stream()), "upconv3d_2x_wgrad")
    return out, gb


def upconv3d_2x_backward_f16x2_supported(shape_x, Cout):
    """m3d_upconv3d_2x_backward_f16x2_supported (host only): upconv3d_2x_dgrad_f16x2 / upconv3d_2x_wgrad_f16x2 take x of shape_x =
    (R, Cin, D, H, W) against Cout output channels: R, D, H, W >= 1, Cin % 32 == 0, Cout % 32 == 0, every tensor below 2^31 elements"""
    if len(shape_x) != 5:
        return False
    R, cin, D, H, W = (int(v) for v in shape_x)
    return bool(lib().m3d_upconv3d_2x_backward_f16x2_supported(R, cin, int(Cout), D, H, W))


def upconv3d_2x_backward_f16x2_plan(direction, R, Cin, Cout, D, H, W):
    """What upconv3d_2x_dgrad_f16x2 / _wgrad_f16x2 (direction "dgrad" / "wgrad") run at the shape (m3d_upconv3d_2x_*_f16x2_plan, host
    only): dict(slices, chain, folds) - the partial sums the reduce launch adds (dgrad: 1), the most MFMAs one accumulator chains
    (<= 384) and the folds of a slice's accumulator into fp32 registers - and for "wgrad" also gb_partials, the partial sums of a bias
    gradient; None where the shape is not supported."""
    if direction not in ("dgrad", "wgrad"):
        raise ValueError("upconv3d_2x_backward_f16x2_plan(%r): 'dgrad' or 'wgrad'" % (direction,))
    keys = ("slices", "chain", "folds") + (("gb_partials",) if direction == "wgrad" else ())
    v = [C.c_int(0) for _ in keys]
    fn = lib().m3d_upconv3d_2x_dgrad_f16x2_plan if direction == "dgrad" else lib().m3d_upconv3d_2x_wgrad_f16x2_plan
    rc = fn(int(R), int(Cin), int(Cout), int(D), int(H), int(W), *[C.byref(a) for a in v])
    if rc == -4:
        return None
    check(rc, "upconv3d_2x_%s_f16x2_plan" % direction)
    return dict(zip(keys, (a.value for a in v)))


def _slots_arg(what, b):
    """an operand bound for the up-conv's f16x2 backward: None (the library sweeps), or ZwConv3d.SLOTS contiguous device floats whose
    largest is the bound; a 1-element bound (ops.absmax) is widened with zeros"""
    if b is None:
        return None
    _need_gpu(b)
    if not (b.dtype == torch.float32 and b.is_contiguous() and b.numel() in (1, ZwConv3d.SLOTS)):
        raise ValueError("%s: a bound is 1 or %d contiguous float32 device values" % (what, ZwConv3d.SLOTS))
    if b.numel() == 1:
        b = torch.nn.functional.pad(b.reshape(1), (0, ZwConv3d.SLOTS - 1))
    return b


def _upconv_mask(what, gy, y):
    if y is None:
        return None
    _need_gpu(y)
    y = _f32c(y)
    if y.shape != gy.shape:
        raise ValueError("%s: y is %s but gy is %s" % (what, tuple(y.shape), tuple(gy.shape)))
    return y


def upconv3d_2x_dgrad_f16x2(gy, weight, y=None, gy_max=None, w_max=None, out=None):
    """upconv3d_2x_dgrad on the f16 matrix cores at fp32 accuracy (m3d_upconv3d_2x_dgrad_f16x2; csrc/upconv3d_bwd_f16.hip): gy
    [R,Cout,2D,2H,2W], weight [Cin,Cout,2,2,2] -> [R,Cin,D,H,W], both read as fp32 and cut while they are staged - no pack, no shuffled
    copy.  y: the output of a relu forward (gy counts only where y > 0, selected before the cut).  gy_max / w_max: [ZwConv3d.SLOTS]
    device floats whose largest bounds the UNMASKED |gy| / |weight| (ZwConv3d.bound_of; a 1-element ops.absmax result is taken too);
    None: the library sweeps that operand.  An unsupported shape is an error: ask upconv3d_2x_backward_f16x2_supported (or
    conv_plan.upconv_backward_kernel).  R == 0 returns zeros without a launch."""
    what = "upconv3d_2x_dgrad_f16x2"
    _need_gpu(gy, weight)
    gy, weight = _f32c(gy), _f32c(weight)
    R, cin, cout, D, H, W = _upconv_dims(what, weight, g=gy)
    y = _upconv_mask(what, gy, y)
    gm, wm = _slots_arg(what, gy_max), _slots_arg(what, w_max)
    _claim(out)
    if out is None:
        out = torch.empty((R, cin, D, H, W), dtype=torch.float32, device=gy.device)
    if tuple(out.shape) != (R, cin, D, H, W) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("%s: out must be a contiguous float32 %s" % (what, (R, cin, D, H, W)))
    if R == 0:
        return out.zero_()
    wsb = lib().m3d_upconv3d_2x_dgrad_f16x2_workspace_bytes(R, cin, cout, D, H, W)
    ws = _workspace(max(wsb, 16), gy.device, "upconv-f16")
    check(lib().m3d_upconv3d_2x_dgrad_f16x2(_ptr(gy), _ptr(y), _ptr(weight), _ptr(out), R, cin, cout, D, H, W, _ptr(gm), _ptr(wm),
                                            _ptr(ws), C.c_size_t(wsb), _stream()), what)
    return out


def upconv3d_2x_wgrad_f16x2(gy, x, y=None, gy_max=None, x_max=None, bias=True, out=None):
    """upconv3d_2x_wgrad on the f16 matrix cores at fp32 accuracy (m3d_upconv3d_2x_wgrad_f16x2): gy [R,Cout,2D,2H,2W], x [R,Cin,D,H,W]
    -> ([Cin,Cout,2,2,2], [Cout] or None without `bias`); the bias gradient is summed from the uncut masked fp32 values.  y and the
    bounds as upconv3d_2x_dgrad_f16x2 (x_max: what the conv before left on x, or a sweep).  R == 0 returns zeros without a launch."""
    what = "upconv3d_2x_wgrad_f16x2"
    _need_gpu(gy, x)
    gy, x = _f32c(gy), _f32c(x)
    if gy.dim() != 5 or x.dim() != 5:
        raise ValueError("%s: gy is %s, x is %s" % (what, tuple(gy.shape), tuple(x.shape)))
    cin, cout = int(x.shape[1]), int(gy.shape[1])
    R, D, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), int(x.shape[4])
    if tuple(gy.shape) != (R, cout, 2 * D, 2 * H, 2 * W):
        raise ValueError("%s: gy is %s, expected %s" % (what, tuple(gy.shape), (R, cout, 2 * D, 2 * H, 2 * W)))
    y = _upconv_mask(what, gy, y)
    gm, xm = _slots_arg(what, gy_max), _slots_arg(what, x_max)
    _claim(out)
    if out is None:
        out = torch.empty((cin, cout, 2, 2, 2), dtype=torch.float32, device=gy.device)
    if tuple(out.shape) != (cin, cout, 2, 2, 2) or not out.is_contiguous() or out.dtype != torch.float32:
        raise ValueError("%s: out must be a contiguous float32 %s" % (what, (cin, cout, 2, 2, 2)))
    gb = torch.empty((cout,), dtype=torch.float32, device=gy.device) if bias else None
    if R == 0:
        return out.zero_(), (gb.zero_() if bias else None)
    wsb = lib().m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(R, cin, cout, D, H, W)
    ws = _workspace(max(wsb, 16), gy.device, "upconv-f16")
    check(lib().m3d_upconv3d_2x_wgrad_f16x2(_ptr(gy), _ptr(y), _ptr(x), _ptr(out), _ptr(gb), R, cin, cout, D, H, W, _ptr(gm), _ptr(xm),
                                            _ptr(ws), C.c_size_t(wsb), _stream()), what)
    return out, gb


class UpConvF16(object):
    """The FORWARD of ConvTranspose3d(kernel 2, stride 2, padding 0) on the f16 matrix cores at fp32 accuracy (csrc/upconv3d_f16.hip: the
    f16x2 cut of ZnConv3d, x cut while it is staged, the weight [Cin, Cout, 2, 2, 2] cut once here), with two epilogues: __call__ writes
    what upconv3d_2x_forward writes; `tail` goes on through ReLU, the 1x1x1 classifier and the sigmoid in the same launch and writes only
    [R, K, 2D, 2H, 2W] (K <= 8).  The operand bound travels as for the f16x2 convs: in_max = the [ZwConv3d.SLOTS] device floats the conv
    before left (None: one ZwConv3d.bound_of sweep of x)."""
    MAX_CLASSES = 8

    @staticmethod
    def supported(weight):
        """weight [Cin, Cout, 2, 2, 2] with Cin % 16 == 0"""
        return (weight.dim() == 5 and tuple(weight.shape[2:]) == (2, 2, 2)
                and lib().m3d_upconv3d_2x_f16x2_packed_bytes(int(weight.shape[0]), int(weight.shape[1])) > 0)

    def __init__(self, weight):
        _need_gpu(weight)
        w = _f32c(weight)
        if not self.supported(w):
            raise ValueError("UpConvF16: weight [Cin, Cout, 2, 2, 2] with Cin %% 16 == 0, got %s" % (tuple(weight.shape),))
        self.cin, self.cout = int(w.shape[0]), int(w.shape[1])
        nbytes = lib().m3d_upconv3d_2x_f16x2_packed_bytes(self.cin, self.cout)
        self.packed = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
        check(lib().m3d_upconv3d_2x_f16x2_pack(_ptr(w), self.cin, self.cout, _ptr(self.packed), _stream()), "upconv3d_2x_f16x2_pack")

    def supports(self, shape):
        """an input of this shape [R, Cin, D, H, W] runs on the kernel (m3d_upconv3d_2x_f16x2_supported)"""
        if len(shape) != 5 or int(shape[1]) != self.cin:
            return False
        R, _, D, H, W = (int(v) for v in shape)
        return bool(lib().m3d_upconv3d_2x_f16x2_supported(R, self.cin, self.cout, D, H, W))

    def _operands(self, x, in_max):
        _need_gpu(x, in_max)
        x = _f32c(x)
        if x.dim() != 5 or int(x.shape[1]) != self.cin:
            raise ValueError("UpConvF16: x is %s, Cin is %d" % (tuple(x.shape), self.cin))
        if in_max is None:
            in_max = ZwConv3d.bound_of(x) if x.numel() else torch.zeros((ZwConv3d.SLOTS,), dtype=torch.float32, device=x.device)
        assert in_max.numel() == ZwConv3d.SLOTS and in_max.dtype == torch.float32
        return x, in_max

    def __call__(self, x, in_max, bias=None, relu=False, out=None):
        x, in_max = self._operands(x, in_max)
        R, _, D, H, W = (int(v) for v in x.shape)
        if bias is not None:
            _need_gpu(bias)
            bias = _f32c(bias)
            assert bias.numel() == self.cout
        _claim(out)
        if out is None:
            out = torch.empty((R, self.cout, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        assert tuple(out.shape) == (R, self.cout, 2 * D, 2 * H, 2 * W) and out.is_contiguous()
        check(lib().m3d_upconv3d_2x_forward_f16x2(_ptr(x), _ptr(self.packed), _ptr(bias), _ptr(out), R, self.cin, self.cout, D, H, W,
                                                  int(bool(relu)), _ptr(in_max), _stream()), "upconv3d_2x_forward_f16x2")
        return out

    def tail(self, x, in_max, up_bias, cls_weight, cls_bias, sigmoid=True, out=None):
        """act(cls_bias[k] + sum_co cls_weight[k, co] relu(upconv(x) + up_bias)[co]) -> [R, K, 2D, 2H, 2W]; cls_weight [K, Cout] or the
        conv's [K, Cout, 1, 1, 1]; act = torch.sigmoid's formula, or the identity (sigmoid=False: the logits)."""
        x, in_max = self._operands(x, in_max)
        R, _, D, H, W = (int(v) for v in x.shape)
        _need_gpu(up_bias, cls_weight, cls_bias)
        cls_weight = _f32c(cls_weight)
        K = int(cls_weight.shape[0])
        if cls_weight.numel() != K * self.cout:
            raise ValueError("UpConvF16.tail: cls_weight is %s, Cout is %d" % (tuple(cls_weight.shape), self.cout))
        up_bias = _f32c(up_bias) if up_bias is not None else None
        cls_bias = _f32c(cls_bias) if cls_bias is not None else None
        assert (up_bias is None or up_bias.numel() == self.cout) and (cls_bias is None or cls_bias.numel() == K)
        _claim(out)
        if out is None:
            out = torch.empty((R, K, 2 * D, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
        assert tuple(out.shape) == (R, K, 2 * D, 2 * H, 2 * W) and out.is_contiguous()
        check(lib().m3d_mask_tail_f16x2(_ptr(x), _ptr(self.packed), _ptr(up_bias), _ptr(cls_weight), _ptr(cls_bias), _ptr(out), R, self.cin,
                                        self.cout, K, D, H, W, int(bool(sigmoid)), _ptr(in_max), _stream()), "mask_tail_f16x2")
        return out


class SplitLinear:
    """nn.Linear weights cut once into three bf16 planes for m3d_linear_bf16x3_forward (fp32 accuracy at the bf16 matrix rate:
    x = xh + xm + xl exactly, six bf16 MFMAs per fp32 product).  `supported(weight)`: K a multiple of 32."""

    @staticmethod
    def supported(weight):
        return weight.dim() == 2 and weight.shape[1] % 32 == 0 and weight.shape[0] >= 64

    def __init__(self, weight, bias=None):
        _need_gpu(weight, bias)
        weight = _f32c(weight)
        self.N, self.K = int(weight.shape[0]), int(weight.shape[1])
        nb = lib().m3d_linear_bf16x3_packed_bytes(self.N, self.K)
        if nb == 0:
            raise ValueError("SplitLinear: K = %d is not a multiple of 32" % self.K)
        self.packed = torch.empty((nb,), dtype=torch.uint8, device=weight.device)
        check(lib().m3d_linear_bf16x3_pack(_ptr(weight), self.N, self.K, _ptr(self.packed), _stream()), "linear_bf16x3_pack")
        self.bias = None if bias is None else _f32c(bias)
        self.weight = weight                    # the many-rows kernel (256 x 256 tiles) cuts the fp32 weight itself
        self.tail_rows = 64                     # <= this many rows past a multiple of 256 go to the fp32 kernel's ragged-tile path
        self.big_rows = 2048                    # from this many rows on (N >= 256): m3d_linear_bf16x3_w32_forward (2560 rows: 2.21 vs 2.35 ms)

    def __call__(self, x, relu=False, out=None, variant=None):
        """variant: None = by shape, "packed" (128 / 256 x 128 tiles on the packed planes), "w32" (256 x 256 tiles, fp32 weight)."""
        _need_gpu(x)
        x = _f32c(x)
        M, K = x.shape
        if K != self.K:
            raise ValueError("SplitLinear: x is [%d,%d] but the weight is [%d,%d]" % (M, K, self.N, self.K))
        _claim(out)
        if out is None:
            out = torch.empty((M, self.N), dtype=torch.float32, device=x.device)
        if M == 0:
            return out
        if variant is None:
            if M <= 32:                                   # a handful of rows: the fp32-input kernel's ragged-tile path (M = 2: 0.09 vs 0.18 ms)
                return linear(x, self.weight, self.bias, relu=relu, out=out)
            variant = "w32" if (M >= self.big_rows and self.N >= 256) else "packed"
            # a few rows past a multiple of the 256-row tile (M = 1281 = 5 x 256 + 1 pads 20 % more rows): those rows go through the
            # fp32-input kernel's ragged-tile path instead (same accuracy class), the rest through full tiles
            rem = M % 256
            if variant == "packed" and M > 512 and 0 < rem <= self.tail_rows:
                self(x[:M - rem], relu=relu, out=out[:M - rem], variant="packed")
                linear(x[M - rem:], self.weight, self.bias, relu=relu, out=out[M - rem:])
                return out
        if variant == "w32":
            wsb = lib().m3d_linear_bf16x3_w32_workspace_bytes(M, self.N, K)
            ws = torch.empty((max(wsb, 16) // 4,), dtype=torch.float32, device=x.device)
            check(lib().m3d_linear_bf16x3_w32_forward(_ptr(x), _ptr(self.weight), _ptr(self.bias), _ptr(out), M, self.N, K, int(bool(relu)),
                                                      _ptr(ws), C.c_size_t(wsb), _stream()), "linear_bf16x3_w32_forward")
            return out
        wsb = lib().m3d_linear_bf16x3_workspace_bytes(M, self.N, K)
        ws = torch.empty((max(wsb, 16) // 4,), dtype=torch.float32, device=x.device)
        check(lib().m3d_linear_bf16x3_forward(_ptr(x), _ptr(self.packed), _ptr(self.bias), _ptr(out), M, self.N, K, int(bool(relu)),
                                              _ptr(ws), C.c_size_t(wsb), _stream()), "linear_bf16x3_forward")
        return out


def absmax(x):
    """max |x| of a float32 CUDA tensor as a 1-element device tensor (m3d_absmax; no host read).  Used as the bound of |RoIAlign
    output| that sets the f16x2 GEMM's operand scale: the RoIAlign output is a convex combination of the feature map's values."""
    _need_gpu(x)
    x = _f32c(x)
    out = torch.empty((1,), dtype=torch.float32, device=x.device)
    check(lib().m3d_absmax(_ptr(x), C.c_longlong(x.numel()), _ptr(out), _stream()), "absmax")
    return out


class SplitLinearF16:
    """nn.Linear on the f16 matrix cores at fp32 accuracy with THREE products per fp32 product (csrc/fc_gemm.hip, "f16x2 split": both
    operands scaled by a power of two and cut into two fp16 numbers, 22 bits; the dropped terms are below the rounding of the fp32
    accumulation).  Weights cut once (4 bytes per element).  __call__(x, relu, out, x_bound, out_bound): x_bound = device floats whose
    largest is >= max|x| - one (ops.absmax of x, or of the feature map the RoIAlign read) or a slot array (ZwConv3d.SLOTS: what the conv
    that produced the feature map, or an earlier call's out_bound, left); None: the library sweeps x itself.  out_bound: a ZEROED
    [ZwConv3d.SLOTS] tensor that receives max|out| from the launch that stores `out` (the next layer's x_bound: no sweep of `out`)."""

    @staticmethod
    def supported(weight):
        return SplitLinear.supported(weight)

    def __init__(self, weight, bias=None):
        _need_gpu(weight, bias)
        weight = _f32c(weight)
        self.N, self.K = int(weight.shape[0]), int(weight.shape[1])
        nb = lib().m3d_linear_f16x2_packed_bytes(self.N, self.K)
        if nb == 0:
            raise ValueError("SplitLinearF16: K = %d is not a multiple of 32" % self.K)
        self.packed = torch.empty((nb,), dtype=torch.uint8, device=weight.device)
        check(lib().m3d_linear_f16x2_pack(_ptr(weight), self.N, self.K, _ptr(self.packed), _stream()), "linear_f16x2_pack")
        self.bias = None if bias is None else _f32c(bias)
        self.weight = weight

    def __call__(self, x, relu=False, out=None, x_bound=None, out_bound=None):
        _need_gpu(x)
        x = _f32c(x)
        M, K = x.shape
        if K != self.K:
            raise ValueError("SplitLinearF16: x is [%d,%d] but the weight is [%d,%d]" % (M, K, self.N, self.K))
        _claim(out)
        if out is None:
            out = torch.empty((M, self.N), dtype=torch.float32, device=x.device)
        if M == 0:
            return out
        if M <= 32:                                       # a handful of rows: the fp32-input kernel's ragged-tile path (out_bound stays zero)
            return linear(x, self.weight, self.bias, relu=relu, out=out)
        if x_bound is not None:
            _need_gpu(x_bound)
            assert x_bound.dtype == torch.float32 and x_bound.numel() in (1, ZwConv3d.SLOTS) and x_bound.is_contiguous()
        if out_bound is not None:
            _need_gpu(out_bound)
            assert out_bound.dtype == torch.float32 and out_bound.numel() == ZwConv3d.SLOTS and out_bound.is_contiguous()
        wsb = lib().m3d_linear_f16x2_workspace_bytes(M, self.N, K)
        ws = torch.empty((wsb // 4,), dtype=torch.float32, device=x.device)
        check(lib().m3d_linear_f16x2_forward_bounds(_ptr(x), _ptr(self.packed), _ptr(self.bias), _ptr(out), M, self.N, K, int(bool(relu)),
                                                    _ptr(x_bound), 0 if x_bound is None else int(x_bound.numel()), _ptr(out_bound),
                                                    _ptr(ws), C.c_size_t(wsb), _stream()), "linear_f16x2_forward")
        return out


def linear_roi_fused(split, features, rois, spatial_scale, relu=False):
    """f-1 A/B: act(RoIAlign3D(features, rois).view(R, -1) @ W.T + b) with the gather inside the GEMM's operand loader
    (m3d_linear_bf16x3_roi_forward; 7^3 bins, sampling grid 2): the [R, C*343] intermediate is never written.  split: SplitLinear of the
    layer.  The product path stays RoIAlign + SplitLinear (two launches): see profiles/r04_f1_ab.json."""
    _need_gpu(features, rois)
    features, rois = _f32c(features), _f32c(rois)
    B, Cc, S, H, W = features.shape
    R = int(rois.shape[0])
    assert split.K == Cc * 343 and rois.shape[1] == 7
    out = torch.empty((R, split.N), dtype=torch.float32, device=features.device)
    if R == 0:
        return out
    tab = torch.empty((R, 42, 4), dtype=torch.int32, device=features.device)
    rb = torch.empty((R,), dtype=torch.int32, device=features.device)
    check(lib().m3d_roi_align3d_tap_tables(_ptr(rois), R, C.c_float(spatial_scale), B, S, H, W, _ptr(tab), _ptr(rb), _stream()), "roi_align3d_tap_tables")
    wsb = lib().m3d_linear_bf16x3_roi_workspace_bytes(R, split.N, split.K)
    ws = torch.empty((max(wsb, 16) // 4,), dtype=torch.float32, device=features.device)
    check(lib().m3d_linear_bf16x3_roi_forward(_ptr(features), B, Cc, S, H, W, _ptr(tab), _ptr(rb), _ptr(split.packed), _ptr(split.bias), _ptr(out),
                                              R, split.N, int(bool(relu)), _ptr(ws), C.c_size_t(wsb), _stream()), "linear_bf16x3_roi_forward")
    return out


def mask_paste3d(masks, channel, boxes_int, shape, thresh=0.5):
    """segm_results' paste (lib/core/test.py:886-945) for all detections at once.  masks [R, C, M, M, M] CUDA fp32; channel [R]
    ints; boxes_int [R, 6] = expand_boxes(ref_boxes, (M+2)/M).astype(int32) (host); shape = (im_s, im_h, im_w).
    Returns uint8 [R, im_s, im_h, im_w] on the device.  The Gaussian taps of skimage's anti-aliasing filter are computed here,
    on the host, exactly as scipy.ndimage does (np.exp, NumPy's pairwise sum), per detection and axis."""
    _need_gpu(masks)
    masks = _f32c(masks)
    R, Cc, M = int(masks.shape[0]), int(masks.shape[1]), int(masks.shape[2])
    S, H, W = (int(v) for v in shape)
    out = torch.empty((R, S, H, W), dtype=torch.uint8, device=masks.device)
    if R == 0:
        return out
    rb = np.ascontiguousarray(boxes_int, dtype=np.int32).reshape(R, 6)
    P = M + 2
    size = np.maximum(rb[:, [5, 4, 3]] - rb[:, [2, 1, 0]] + 1, 1).astype(np.float64)           # (s, h, w)
    sigma = np.maximum(0, (float(P) / size - 1) / 2)                                           # skimage: (in/out - 1) / 2
    radius = np.where(sigma > 1e-15, (4.0 * sigma + 0.5).astype(np.int64), 0).astype(np.int32)  # scipy: int(truncate * sd + 0.5)
    ws_ = int(radius.max()) + 1
    weights = np.zeros((R, 3, ws_), dtype=np.float64)
    for (r, a) in zip(*np.nonzero(radius)):
        rad, sg = int(radius[r, a]), float(sigma[r, a])
        x = np.arange(-rad, rad + 1)
        phi = np.exp(-0.5 / (sg * sg) * x ** 2)
        phi = phi / phi.sum()
        weights[r, a, :rad + 1] = phi[rad:]                                                    # symmetric: [d] = distance d
    dev = masks.device
    d_ch = torch.from_numpy(np.ascontiguousarray(channel, dtype=np.int32)).to(dev)
    d_rb = torch.from_numpy(rb).to(dev)
    d_rad = torch.from_numpy(np.ascontiguousarray(radius)).to(dev)
    d_w = torch.from_numpy(weights).to(dev)
    wsb = lib().m3d_mask_paste3d_workspace_bytes(R, M)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib().m3d_mask_paste3d(_ptr(masks), R, Cc, M, _ptr(d_ch), _ptr(d_rb), _ptr(d_rad), _ptr(d_w), ws_, C.c_float(thresh),
                                 S, H, W, _ptr(out), _ptr(ws), C.c_size_t(wsb), _stream()), "mask_paste3d")
    return out


def norm1(vol, f32_arith=True, out=None, return_stats=False):
    """mask = vol > 0; (vol - mean(vol[mask])) / std(vol[mask]) on the device -> fp32 tensor of vol's shape.
    vol: uint16 (raw) or float32 CUDA tensor.  f32_arith=True mirrors prep_im_for_blob (blob.py:179-184, float32
    arithmetic); False mirrors infer_simple.py:180-183 (float64, rounded to fp32 once)."""
    _need_gpu(vol)
    vol = vol.contiguous()
    if vol.dtype not in (torch.uint16, torch.float32):
        raise TypeError("norm1 takes uint16 or float32 volumes")
    _claim(out)
    if out is None:
        out = torch.empty(vol.shape, dtype=torch.float32, device=vol.device)
    wsb = lib().m3d_norm1_workspace_bytes()
    ws = torch.empty((wsb // 8,), dtype=torch.float64, device=vol.device)
    stats = torch.empty((3,), dtype=torch.float64, device=vol.device) if return_stats else None
    check(lib().m3d_norm1(_ptr(vol), 0 if vol.dtype == torch.uint16 else 1, C.c_int64(vol.numel()), int(bool(f32_arith)),
                          _ptr(out), _ptr(stats), _ptr(ws), C.c_size_t(wsb), _stream()), "norm1")
    return (out, stats) if return_stats else out


def norm1_batched(vols, f32_arith=True, out=None):
    """norm1 of every volume of a batch [B, ...] with its own statistics, one launch per pass for the whole batch."""
    _need_gpu(vols)
    vols = vols.contiguous()
    if vols.dtype not in (torch.uint16, torch.float32):
        raise TypeError("norm1 takes uint16 or float32 volumes")
    B = vols.shape[0]
    n = vols[0].numel()
    _claim(out)
    if out is None:
        out = torch.empty(vols.shape, dtype=torch.float32, device=vols.device)
    assert out.is_contiguous() and out.numel() == vols.numel() and out.dtype == torch.float32
    wsb = lib().m3d_norm1_workspace_bytes() * B
    ws = torch.empty((wsb // 8,), dtype=torch.float64, device=vols.device)
    check(lib().m3d_norm1_batched(_ptr(vols), 0 if vols.dtype == torch.uint16 else 1, B, C.c_int64(n), int(bool(f32_arith)),
                                  _ptr(out), None, _ptr(ws), C.c_size_t(wsb), _stream()), "norm1_batched")
    return out


def norm1_stats(vols, batch=None):
    """mean, std, count of vol[vol > 0] without the normalised volume: fp64 [3] (batch=None: `vols` is one volume), or fp64 [batch, 3] for
    `batch` volumes of equal size stacked in `vols`.  The bits ops.norm1(..., return_stats=True) reports."""
    _need_gpu(vols)
    vols = vols.contiguous()
    if vols.dtype not in (torch.uint16, torch.float32):
        raise TypeError("norm1 takes uint16 or float32 volumes")
    B = 1 if batch is None else int(batch)
    if B < 1 or vols.numel() % B:
        raise M3DError("norm1_stats: %d elements do not make %d volumes" % (vols.numel(), B))
    wsb = lib().m3d_norm1_workspace_bytes() * B
    ws = torch.empty((wsb // 8,), dtype=torch.float64, device=vols.device)
    stats = torch.empty((B, 3), dtype=torch.float64, device=vols.device)
    check(lib().m3d_norm1_stats(_ptr(vols), 0 if vols.dtype == torch.uint16 else 1, B, C.c_int64(vols.numel() // B), _ptr(stats),
                                _ptr(ws), C.c_size_t(wsb), _stream()), "norm1_stats")
    return stats[0] if batch is None else stats


# ------------------------------------------------------------------ training samples (csrc/train_sample.hip)
def train_sample(images, in_size, need_crop, seeds, max_boxes, fixed_origin=None, data=None, meta=None, boxes_out=None, score=None):
    """m3d_train_sample: the normalised crops and ground-truth boxes of a minibatch, from volumes resident on the device, on the current
    stream and without a host round trip.

    images: per image (vol, stats, boxes, start_max): vol a contiguous CUDA uint16 / float32 [D,H,W] tensor, stats its fp64 [3] statistics
    (norm1_stats), boxes CUDA fp32 [K,6], start_max host (x, y, z).  in_size (s, h, w); seeds: one int per image; fixed_origin: None or
    per image (x, y, z).  data: None, or the contiguous fp32 tensor of B s h w elements to write; meta: None, or a contiguous int32 tensor
    of B (8 + max_boxes) elements that receives info and keep side by side (one copy brings both to the host); boxes_out, score: None, or
    the contiguous fp32 / fp64 tensors of B max_boxes 6 / B elements to write.
    Returns data fp32 [B,1,s,h,w], boxes fp32 [B,max_boxes,6], keep int32 [B,max_boxes], info int32 [B,8], score fp64 [B]."""
    B = len(images)
    s, h, w = (int(v) for v in in_size)
    arr = (TrainImage * max(B, 1))()
    dev = None
    for i, (vol, stats, boxes, start_max) in enumerate(images):
        _need_gpu(vol, stats, boxes)
        if vol.dtype not in (torch.uint16, torch.float32) or vol.dim() != 3 or not vol.is_contiguous():
            raise M3DError("train_sample: volume %d must be a contiguous uint16 or float32 [D,H,W] tensor" % i)
        if stats.dtype != torch.float64 or stats.numel() != 3 or not stats.is_contiguous():
            raise M3DError("train_sample: statistics %d must be a contiguous fp64 [3] tensor" % i)
        if boxes.dtype != torch.float32 or boxes.dim() != 2 or boxes.shape[1] != 6 or not boxes.is_contiguous():
            raise M3DError("train_sample: boxes %d must be a contiguous fp32 [K,6] tensor" % i)
        dev = vol.device
        e = arr[i]
        e.vol, e.stats, e.boxes, e.dtype = vol.data_ptr(), stats.data_ptr(), boxes.data_ptr(), 0 if vol.dtype == torch.uint16 else 1
        e.depth, e.height, e.width, e.num_boxes = int(vol.shape[0]), int(vol.shape[1]), int(vol.shape[2]), int(boxes.shape[0])
        e.start_max[0], e.start_max[1], e.start_max[2] = (int(v) for v in start_max)
    if dev is None:
        raise M3DError("train_sample: no images")
    max_boxes = int(max_boxes)
    if data is None:
        data = torch.empty((B, 1, s, h, w), dtype=torch.float32, device=dev)
    elif not data.is_cuda or data.dtype != torch.float32 or data.numel() != B * s * h * w or not data.is_contiguous():
        raise M3DError("train_sample: data must be a contiguous CUDA fp32 tensor of %d elements" % (B * s * h * w))
    _claim(data)
    if meta is None:
        meta = torch.empty((B * (8 + max_boxes),), dtype=torch.int32, device=dev)
    elif not meta.is_cuda or meta.dtype != torch.int32 or meta.numel() != B * (8 + max_boxes) or not meta.is_contiguous():
        raise M3DError("train_sample: meta must be a contiguous CUDA int32 tensor of %d elements" % (B * (8 + max_boxes)))
    info, keep = meta.view(-1)[:B * 8].view(B, 8), meta.view(-1)[B * 8:].view(B, max_boxes)
    if boxes_out is None:
        boxes_out = torch.empty((B, max_boxes, 6), dtype=torch.float32, device=dev)
    elif not boxes_out.is_cuda or boxes_out.dtype != torch.float32 or boxes_out.numel() != B * max_boxes * 6 or not boxes_out.is_contiguous():
        raise M3DError("train_sample: boxes_out must be a contiguous CUDA fp32 tensor of %d elements" % (B * max_boxes * 6))
    if score is None:
        score = torch.empty((B,), dtype=torch.float64, device=dev)
    elif not score.is_cuda or score.dtype != torch.float64 or score.numel() != B or not score.is_contiguous():
        raise M3DError("train_sample: score must be a contiguous CUDA fp64 tensor of %d elements" % B)
    size = (C.c_int * 3)(s, h, w)
    sd = (C.c_uint64 * max(B, 1))(*[int(v) & (2 ** 64 - 1) for v in seeds]) if seeds is not None else None
    fx = None
    if fixed_origin is not None:
        flat = [int(v) for o in fixed_origin for v in o]
        if len(flat) != 3 * B:
            raise M3DError("train_sample: fixed_origin needs (x, y, z) per image")
        fx = (C.c_int * (3 * B))(*flat)
    if sd is not None and len(seeds) != B:
        raise M3DError("train_sample: one seed per image")
    check(lib().m3d_train_sample(arr, B, size, int(bool(need_crop)), sd, fx, max_boxes, _ptr(data), _ptr(boxes_out), _ptr(keep), _ptr(info),
                                 _ptr(score), None, None, _stream()), "train_sample")
    return data.view(B, 1, s, h, w), boxes_out.view(B, max_boxes, 6), keep, info, score.view(B)


# ------------------------------------------------------------------ Otsu 2D
def otsu2d_batch(image, prm, offsets, max_gray_range=4096):
    """image, prm: flat uint16 CUDA tensors (crops concatenated); offsets int64 [R+1] CUDA.
    Returns (mask uint8 flat, kb int32 [R,2], status int32 [R])."""
    _need_gpu(image, prm, offsets)
    assert image.dtype == torch.uint16 and prm.dtype == torch.uint16 and offsets.dtype == torch.int64
    R = offsets.numel() - 1
    mask = torch.empty(image.shape, dtype=torch.uint8, device=image.device)
    kb = torch.empty((R, 2), dtype=torch.int32, device=image.device)          # otsu_eval_kernel writes both for every RoI, on every path
    status = torch.empty((R,), dtype=torch.int32, device=image.device)
    wsb = lib().m3d_otsu2d_workspace_bytes(R, int(max_gray_range))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=image.device)
    check(lib().m3d_otsu2d_batch(_ptr(image), _ptr(prm), _ptr(offsets), R, int(max_gray_range), _ptr(mask), _ptr(kb),
                                 _ptr(status), _ptr(ws), C.c_size_t(wsb), _stream()), "otsu2d_batch")
    return mask, kb, status


# ------------------------------------------------------------------ PRM window kernels
def conv3d_windowed(packed, x, full, full_off, origins):
    """Batched same-conv on cropped windows + fused (full[co, origin+pos] - off) multiply (m3d_conv3d_forward_windowed)."""
    _need_gpu(x, full, origins)
    x = _f32c(x)
    B, Cin, D, H, W = x.shape
    assert Cin == packed.cin and full.shape[0] == packed.cout and full.dim() == 4 and full.is_contiguous()
    assert origins.dtype == torch.int32 and origins.shape == (B, 3) and origins.is_contiguous()
    out = torch.empty((B, packed.cout, D, H, W), dtype=torch.float32, device=x.device)
    check(lib().m3d_conv3d_forward_windowed(_ptr(x), _ptr(packed.packed), _ptr(out), B, Cin, packed.cout, D, H, W, packed.k,
                                            _ptr(full), _ptr(full_off), _ptr(origins), full.shape[1], full.shape[2],
                                            full.shape[3], _stream()), "conv3d_forward_windowed")
    return out


class SmallWindowDgrad:
    """Backward-data of a 3^3 conv with relu(W) on batches of 3^3 / 5^3 / 7^3 windows, all peaks in one dense GEMM
    (csrc/prm_small.hip); weight = the forward conv's [cout, cin, 3, 3, 3], packed once."""
    SIZES = (3, 5, 7)
    F16_MAX_PEAKS = 65535                                   # peaks per m3d_prm_small_dgrad_f16 launch (the library refuses more)

    def __init__(self, weight, f16=True):
        """f16 (round 6, default where the forward conv's cout is a multiple of 16): the f16x2 split on v_mfma_f32_32x32x16_f16 (csrc/
        prm_small_f16.hip: two scaled fp16 pieces per operand, three products, per-peak gradient scales) instead of the fp32 MFMA GEMM."""
        _need_gpu(weight)
        w = _f32c(weight)
        assert w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3)
        self.cout_fwd, self.cin_fwd = int(w.shape[0]), int(w.shape[1])
        self.f16 = bool(f16) and bool(lib().m3d_prm_small_dgrad_f16_supported(self.cout_fwd, self.cin_fwd))
        if self.f16:
            nbytes = lib().m3d_prm_small_dgrad_f16_packed_bytes(self.cout_fwd, self.cin_fwd)
            self.packed = torch.empty((nbytes // 4,), dtype=torch.float32, device=w.device)
            check(lib().m3d_prm_small_dgrad_f16_pack(_ptr(w), self.cout_fwd, self.cin_fwd, _ptr(self.packed), _stream()), "prm_small_dgrad_f16_pack")
            return
        nbytes = lib().m3d_prm_small_dgrad_packed_bytes(self.cout_fwd, self.cin_fwd)
        self.packed = torch.empty((nbytes // 4,), dtype=torch.float32, device=w.device)
        check(lib().m3d_prm_small_dgrad_pack(_ptr(w), self.cout_fwd, self.cin_fwd, _ptr(self.packed), _stream()), "prm_small_dgrad_pack")

    def __call__(self, gn, full, full_off, origins):
        """gn [P, cout_fwd, n, n, n]; full [cin_fwd, D, H, W]; origins int32 [P,3] -> [P, cin_fwd, n, n, n]."""
        _need_gpu(gn, full, full_off, origins)
        gn = _f32c(gn)
        P, Cc, n = gn.shape[0], gn.shape[1], gn.shape[2]
        assert Cc == self.cout_fwd and n in self.SIZES and full.shape[0] == self.cin_fwd
        out = torch.empty((P, self.cin_fwd, n, n, n), dtype=torch.float32, device=gn.device)
        if self.f16:
            # at most F16_MAX_PEAKS peaks per launch: a peak's rows depend only on its own window and scale, so a split batch computes the
            # whole batch's values bit for bit
            full = _f32c(full)
            for p0 in range(0, P, self.F16_MAX_PEAKS):
                p1 = min(P, p0 + self.F16_MAX_PEAKS)
                wsb = lib().m3d_prm_small_dgrad_f16_workspace_bytes(p1 - p0)
                ws = torch.empty((wsb // 4,), dtype=torch.float32, device=gn.device)
                check(lib().m3d_prm_small_dgrad_f16(_ptr(gn[p0:p1]), _ptr(self.packed), p1 - p0, self.cout_fwd, self.cin_fwd, n, _ptr(full),
                                                    _ptr(full_off), _ptr(origins[p0:p1]), full.shape[1], full.shape[2], full.shape[3],
                                                    _ptr(out[p0:p1]), _ptr(ws), C.c_size_t(wsb), _stream()), "prm_small_dgrad_f16")
            return out
        check(lib().m3d_prm_small_dgrad(_ptr(gn), _ptr(self.packed), P, self.cout_fwd, self.cin_fwd, n, _ptr(_f32c(full)), _ptr(full_off),
                                        _ptr(origins), full.shape[1], full.shape[2], full.shape[3], _ptr(out), _stream()),
              "prm_small_dgrad")
        return out


def prm_seed(peaks, prob, norm_cls, w_cls, h, h_off, return_origin=False):
    """peaks int32 [P,4] (a,s,h,w); prob/norm_cls [A,S,H,W]; w_cls [A,C]; h [C,S,H,W] -> [P,C,1,1,1] (+ with return_origin the peaks'
    (s,h,w) as int32 [P,3], written by the same launch)."""
    _need_gpu(peaks, prob, norm_cls, w_cls, h, h_off)
    P = peaks.shape[0]
    A, S, H, W = prob.shape
    Cc = h.shape[0]
    out = torch.empty((P, Cc, 1, 1, 1), dtype=torch.float32, device=prob.device)
    org = torch.empty((P, 3), dtype=torch.int32, device=prob.device) if return_origin else None
    check(lib().m3d_prm_seed_ex(_ptr(peaks), P, _ptr(prob), _ptr(norm_cls), _ptr(w_cls), _ptr(h), _ptr(h_off), A, Cc, S, H, W,
                                _ptr(out), _ptr(org), _stream()), "prm_seed")
    return (out, org) if return_origin else out


class _StagingRing:
    """Small host arrays (index lists, box tables, offsets) on their way to the device: a ring of pinned 64 KB slots, each guarded by
    the event of its last copy.  `torch.from_numpy(a).to(device)` from pageable memory is a BLOCKING copy that first waits for
    everything queued on the stream - one idle gap on the GPU per call (tools/prm_timeline.sh showed 20-70 us each)."""
    SLOT = 1 << 16

    def __init__(self, n=32):
        self.pool = torch.empty((n * self.SLOT,), dtype=torch.uint8).pin_memory()       # ONE pinning call (each costs milliseconds)
        self.slots = [self.pool[k * self.SLOT:(k + 1) * self.SLOT] for k in range(n)]
        self.events, self.i, self.n, self.big = [None] * n, 0, n, []
        self.lock = threading.Lock()       # slot choice + fill + copy + event are one critical section: drivers own worker threads

    def put(self, arr, device):
        arr = np.ascontiguousarray(arr)
        nb = arr.nbytes
        dt = torch.from_numpy(np.empty((0,), arr.dtype)).dtype
        out = torch.empty(arr.shape, dtype=dt, device=device)
        if nb == 0:
            return out
        with self.lock:
            return self._put_locked(arr, nb, out)

    def _put_locked(self, arr, nb, out):
        if nb > self.SLOT:                                     # big tables: a one-off pinned buffer
            t = torch.from_numpy(arr).pin_memory()
            out.copy_(t, non_blocking=True)
            ev = torch.cuda.Event(); ev.record()
            self.big = [(b, e) for b, e in self.big if not e.query()] + [(t, ev)]
            return out
        k = self.i % self.n
        self.i += 1
        if self.events[k] is not None:
            self.events[k].synchronize()                       # n copies ago: long done
        slot = self.slots[k]
        slot.numpy()[:nb] = arr.reshape(-1).view(np.uint8)
        out.view(torch.uint8).reshape(-1).copy_(slot[:nb], non_blocking=True)
        ev = torch.cuda.Event(); ev.record()
        self.events[k] = ev
        return out


_staging = {}


def upload(arr, device="cuda"):
    """Host ndarray -> device tensor of the same dtype/shape through pinned staging, asynchronous on the current stream."""
    key = str(device)
    ring = _staging.get(key)
    if ring is None:
        ring = _staging[key] = _StagingRing()
    return ring.put(arr, device)


def upload_packed(arrays, device="cuda"):
    """Several small host arrays -> device tensors through ONE staged copy (each array at a 16-byte aligned offset of one buffer)."""
    arrays = [np.ascontiguousarray(a) for a in arrays]
    offs, total = [], 0
    for a in arrays:
        offs.append(total)
        total += (a.nbytes + 15) // 16 * 16
    host = np.zeros((max(total, 16),), np.uint8)
    for a, o in zip(arrays, offs):
        host[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
    dev = upload(host, device)
    out = []
    for a, o in zip(arrays, offs):
        dt = torch.from_numpy(np.empty((0,), a.dtype)).dtype
        out.append(dev[o:o + a.nbytes].view(dt).view(a.shape) if a.nbytes else torch.empty(a.shape, dtype=dt, device=device))
    return out


class PinnedPool:
    """Pinned host buffers of one size, handed out per call and returned after the read: any number of tiles may be in flight
    (double-buffered volume drivers) without one overwriting another's mirror.  Pinning is a slow driver call, hence the pool."""

    def __init__(self):
        self.free = {}
        self.lock = threading.Lock()

    def take(self, nbytes):
        with self.lock:
            lst = self.free.setdefault(int(nbytes), [])
            if lst:
                return lst.pop()
        fresh = [torch.empty((int(nbytes),), dtype=torch.uint8).pin_memory() for _ in range(2)]
        with self.lock:
            self.free[int(nbytes)].append(fresh[1])
        return fresh[0]

    def give(self, buf):
        with self.lock:
            self.free.setdefault(int(buf.numel()), []).append(buf)


_peak_pool = PinnedPool()


def prm_select_peaks(dets, keep_idx, count, peak_threshold, A, fmap_shape, cap=None, prob=None):
    """Device-side peak selection (peak_response_mapping_3d.py:124-139,161-163): dets [rows,7] (class 1's kept detections), keep_idx
    int64 [rows], count int32 [1] (all on the device) -> dict(num int32 [1], peaks int32 [cap,4] = (a,s,h,w), dets f32 [cap,7]) on the
    device plus `host`: a pinned mirror the SAME kernel writes (host["num"] int32 [1], host["peaks"], host["dets"] as NumPy views),
    valid once the returned `event` has completed; call `release()` after reading it.  No host synchronisation here.
    prob ([A,S,H,W], the class response map): the mirror also carries host["dead"] int32 [cap] - 1 where the peak's sigmoid derivative is
    exactly 0 (a saturated score): its back-propagated map is all zero and the engine skips it."""
    _need_gpu(dets, keep_idx, count)
    assert dets.dtype == torch.float32 and dets.is_contiguous() and dets.dim() == 2 and dets.shape[1] == 7
    assert keep_idx.dtype == torch.int64 and keep_idx.is_contiguous() and count.dtype == torch.int32
    rows = int(dets.shape[0])
    cap = int(cap or rows)
    S, H, W = (int(v) for v in fmap_shape)
    dev = dets.device
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    peaks = torch.empty((cap, 4), dtype=torch.int32, device=dev)
    out = torch.empty((cap, 7), dtype=torch.float32, device=dev)
    capb = max(cap, fused_max_boxes())                      # ONE buffer size for every tile (a new size would pin new memory)
    buf = _peak_pool.take(64 + capb * 48)
    base = buf.data_ptr()
    if prob is not None:
        _need_gpu(prob)
        assert prob.dtype == torch.float32 and prob.is_contiguous() and tuple(prob.shape[-4:]) == (int(A), S, H, W)
    check(lib().m3d_prm_select_peaks_ex(_ptr(dets), _ptr(keep_idx), _ptr(count), rows, C.c_float(np.float32(peak_threshold)), int(A), S, H, W,
                                        cap, _ptr(num), _ptr(peaks), _ptr(out), C.c_void_p(base), C.c_void_p(base + 64),
                                        C.c_void_p(base + 64 + capb * 16), _ptr(prob), None,
                                        C.c_void_p(base + 64 + capb * 44) if prob is not None else None, _stream()), "prm_select_peaks")
    ev = torch.cuda.Event()
    ev.record()
    hb = buf.numpy()
    host = dict(num=hb[:4].view(np.int32), peaks=hb[64:64 + cap * 16].view(np.int32).reshape(cap, 4),
                dets=hb[64 + capb * 16:64 + capb * 16 + cap * 28].view(np.float32).reshape(cap, 7),
                dead=hb[64 + capb * 44:64 + capb * 44 + cap * 4].view(np.int32) if prob is not None else None)
    return dict(num=num, peaks=peaks, dets=out, host=host, event=ev, release=lambda: _peak_pool.give(buf))


def strip_geometry(n, mode, P):
    """(pitch, lead, L) of the strip layout of P windows n voxels wide (include/m3d.h: m3d_prm_strip_geometry); mode 1 / True: pitch
    n + 1 (exactly-local F(2x2,3x3)), mode 2: quad-aligned for F(2x4,3x3)."""
    pitch, lead = C.c_int32(0), C.c_int32(0)
    L = lib().m3d_prm_strip_geometry(int(n), int(mode), int(P), C.byref(pitch), C.byref(lead))
    return pitch.value, lead.value, int(L)


PRM_PREPARE_KERNELS = ("element", "quad<8>", "quad<16>", "quad<32>", "pool")
PRM_STEM_DGRAD_LAYOUTS = ("<4,8>", "<5,6>")


def prm_prepare_plan(channels, num_peaks, up_size, pool, border, out_strip=0, out_slab=False, depth=1):
    """The kernel prm_prepare launches for this shape (m3d_prm_prepare_plan, host only; an output that is 16-byte aligned, as every
    torch allocation is): one of PRM_PREPARE_KERNELS, or None where the library refuses the shape."""
    rc = lib().m3d_prm_prepare_plan(int(channels), int(num_peaks), int(up_size), int(bool(pool)), int(border), int(out_strip),
                                    int(bool(out_slab)), int(depth))
    return PRM_PREPARE_KERNELS[rc] if rc >= 0 else None


def prm_stem_dgrad_plan(win):
    """The thread layout prm_stem_dgrad launches for win^3 windows (m3d_prm_stem_dgrad_plan, host only): one of PRM_STEM_DGRAD_LAYOUTS."""
    rc = lib().m3d_prm_stem_dgrad_plan(int(win))
    check(min(rc, 0), "prm_stem_dgrad_plan")
    return PRM_STEM_DGRAD_LAYOUTS[rc]


def prm_prepare(gup, origin_up, pool, border, argmax, xnext, scale, norm, in_strip=False, out_strip=False, up_off=None, dims=None,
                in_slab=False, out_slab=False, peak_max=False):
    """gup [P,C,U,U,U]; xnext [C,UD,UH,UW]; norm [C,D,H,W] -> (window [P,C,Wn,Wn,Wn], origin int32 [P,3]).
    Strip layout (in_strip / out_strip): the P windows side by side along x with one separator column after each,
    [C,n,n,P*(n+1)] - what the Winograd kernel convolves as one wide volume; dims = (P, C, U) is then required.
    up_off (1-element tensor): gup is the bare backward-data of the layer above and its PreHook multiply by (xnext - up_off)
    (peak_backprop_3d.py:16-18) is applied here.
    in_slab / out_slab (strips only): the strip stores the planes of the layer's map - [C, xnext depth, U, L] / [C, norm depth, Wn, L] -
    instead of each window's (m3d.h: depth-clipped strips)."""
    _need_gpu(gup, origin_up, xnext, norm)
    P, Cc, U = dims if dims is not None else (gup.shape[0], gup.shape[1], gup.shape[2])
    in_strip, out_strip = int(in_strip), int(out_strip)                       # 0 batch-major, 1 strip (pitch n + 1), 2 quad-aligned strip
    in_slab, out_slab = bool(in_slab) and bool(in_strip), bool(out_slab) and bool(out_strip)
    assert tuple(gup.shape) == ((Cc, xnext.shape[1] if in_slab else U, U, strip_geometry(U, in_strip, P)[2]) if in_strip else (P, Cc, U, U, U))
    Wn = (2 if pool else 1) * U + 2 * border
    out = torch.empty((Cc, norm.shape[1] if out_slab else Wn, Wn, strip_geometry(Wn, out_strip, P)[2]) if out_strip else (P, Cc, Wn, Wn, Wn),
                      dtype=torch.float32, device=gup.device)
    oo = torch.empty((P, 3), dtype=torch.int32, device=gup.device)
    # peak_max: the launch also leaves the largest |value| of every peak's window on the output tensor (`_m3d_peak_max` [P]): the per-window
    # operand bounds of ZwConv3d.strip
    pm = torch.empty((P, 32), dtype=torch.float32, device=gup.device) if peak_max else None      # (one cache line per peak, value in column 0)
    check(lib().m3d_prm_prepare_ex3(_ptr(gup), _ptr(origin_up), P, Cc, U, int(bool(pool)), int(border), _ptr(argmax), _ptr(xnext),
                                    xnext.shape[1], xnext.shape[2], xnext.shape[3], _ptr(scale), _ptr(norm), norm.shape[1],
                                    norm.shape[2], norm.shape[3], in_strip, int(in_slab), out_strip, int(out_slab), _ptr(up_off), _ptr(out),
                                    _ptr(oo), _ptr(pm) if pm is not None else None, _stream()), "prm_prepare")
    if pm is not None:
        out._m3d_peak_max = pm
    return out, oo


def prm_stem_prepare_weights(weight):
    """weight [C,1,5,5,5] -> [C,125] flipped relu(W) for prm_stem_dgrad."""
    _need_gpu(weight)
    weight = _f32c(weight)
    Cc = weight.shape[0]
    wf = torch.empty((Cc, 125), dtype=torch.float32, device=weight.device)
    check(lib().m3d_prm_stem_prepare_weights(_ptr(weight), Cc, _ptr(wf), _stream()), "prm_stem_prepare_weights")
    return wf


def prm_stem_dgrad(gn, weight, data, data_off, origins):
    """gn [P,C,Wn,Wn,Wn]; weight = prm_stem_prepare_weights(conv1a.weight); data [D,H,W] ->
    (windows [P,Wn,Wn,Wn] clamped, sums [P])."""
    _need_gpu(gn, weight, data, data_off, origins)
    assert weight.dim() == 2 and weight.shape[1] == 125
    P, Cc, Wn = gn.shape[0], gn.shape[1], gn.shape[2]
    out = torch.empty((P, Wn, Wn, Wn), dtype=torch.float32, device=gn.device)
    sums = torch.empty((P,), dtype=torch.float32, device=gn.device)
    check(lib().m3d_prm_stem_dgrad(_ptr(gn), _ptr(weight), _ptr(data), _ptr(data_off), _ptr(origins), P, Cc, Wn, data.shape[0],
                                   data.shape[1], data.shape[2], _ptr(out), _ptr(sums), _stream()), "prm_stem_dgrad")
    return out, sums


def prm_den_pool(argmax, xnext, norm):
    """Peak-independent denominator map of a conv + MaxPool3d(2,2) layer: argmax uint8 / xnext [C,UD,UH,UW] (pool argmax and
    pooled activation), norm [C,D,H,W] (norm conv) -> den [C,UD,UH,UW] = |N| + 1e-10 at the argmax child where xnext > 0 and
    N >= 1e-10, else 0 (peak_backprop_3d.py:30-33 + ReLU / max-unpool routing)."""
    _need_gpu(argmax, xnext, norm)
    assert argmax.dtype == torch.uint8 and argmax.shape == xnext.shape
    Cc, UD, UH, UW = xnext.shape
    den = torch.empty_like(xnext)
    check(lib().m3d_prm_den_pool(_ptr(argmax.contiguous()), _ptr(_f32c(xnext)), _ptr(_f32c(norm)), Cc, UD, UH, UW, norm.shape[1],
                                 norm.shape[2], norm.shape[3], _ptr(den), _stream()), "prm_den_pool")
    return den


def prm_stem_mfma_weights(weight):
    """conv1a.weight [32,1,5,5,5] -> MFMA A-operand pack [80,64] of the tap-flipped relu(W) for prm_stem_dgrad_fused."""
    _need_gpu(weight)
    weight = _f32c(weight)
    assert tuple(weight.shape[1:]) == (1, 5, 5, 5)
    wa = torch.empty((80, 64), dtype=torch.float32, device=weight.device)
    check(lib().m3d_prm_stem_mfma_prepare_weights(_ptr(weight), weight.shape[0], _ptr(wa), _stream()), "prm_stem_mfma_prepare_weights")
    return wa


def prm_stem_dgrad_fused_supported(channels, up_size):
    return bool(lib().m3d_prm_stem_dgrad_fused_supported(int(channels), int(up_size)))


def prm_stem_dgrad_fused(gup, origin_up, den, argmax, scale, wa, data, data_off, strip=False, xnext=None, up_off=None, dims=None, slab=False):
    """Max-unpool + ReLU + BN + PostHook + backward-data of conv1a + PreHook in one MFMA kernel.  gup [P,32,U,U,U] (gradient
    w.r.t. the pooled stem output; strip=True: [32,U,U,P*(U+1)], dims = (P, 32, U)), origin_up int32 [P,3] (pooled
    coordinates), den = prm_den_pool(...), argmax uint8 [32,UD,UH,UW], scale [32] or None, wa = prm_stem_mfma_weights(W),
    data [D,H,W]; xnext + up_off: gup is the bare backward-data of conv2a, multiplied here by (xnext - up_off) ->
    (windows [P,Wn,Wn,Wn] clamped (Wn = 2U + 4), sums [P], origins int32 [P,3])."""
    _need_gpu(gup, origin_up, den, argmax, wa, data, data_off)
    P, Cc, U = dims if dims is not None else (gup.shape[0], gup.shape[1], gup.shape[2])
    strip = int(strip)
    slab = bool(slab) and bool(strip)                                            # gup stores the pooled layer's planes (den.shape[1] of them)
    assert tuple(gup.shape) == ((Cc, den.shape[1] if slab else U, U, strip_geometry(U, strip, P)[2]) if strip else (P, Cc, U, U, U)) and gup.is_contiguous()
    assert (xnext is None) == (up_off is None)
    Wn = 2 * U + 4
    out = torch.empty((P, Wn, Wn, Wn), dtype=torch.float32, device=gup.device)
    sums = torch.empty((P,), dtype=torch.float32, device=gup.device)
    oo = torch.empty((P, 3), dtype=torch.int32, device=gup.device)
    check(lib().m3d_prm_stem_dgrad_fused_ex2(_ptr(gup), strip, int(slab), _ptr(xnext), _ptr(up_off), _ptr(origin_up), P, Cc, U,
                                            _ptr(den), _ptr(argmax), _ptr(scale), den.shape[1], den.shape[2], den.shape[3],
                                            _ptr(wa), _ptr(data), _ptr(data_off), data.shape[0], data.shape[1], data.shape[2],
                                            _ptr(out), _ptr(sums), _ptr(oo), _stream()), "prm_stem_dgrad_fused")
    return out, sums, oo


def conv3d_stem5_dgrad_weights(weight):
    """weight [C,1,5,5,5] -> [C,125] tap-flipped (no ReLU) for conv3d_stem5_dgrad."""
    _need_gpu(weight)
    weight = _f32c(weight)
    assert tuple(weight.shape[1:]) == (1, 5, 5, 5)
    wf = torch.empty((weight.shape[0], 125), dtype=torch.float32, device=weight.device)
    check(lib().m3d_conv3d_stem5_prepare_dgrad_weights(_ptr(weight), weight.shape[0], _ptr(wf), _stream()), "stem5_prepare_dgrad_weights")
    return wf


def conv3d_stem5_dgrad(grad_out, wf):
    """Backward-data of the 5^3 / Cin=1 stem conv: grad_out [B,C,D,H,W], wf = conv3d_stem5_dgrad_weights(W) -> [B,1,D,H,W]."""
    _need_gpu(grad_out, wf)
    grad_out = _f32c(grad_out)
    B, Cc, D, H, W = grad_out.shape
    assert wf.shape == (Cc, 125)
    gin = torch.empty((B, 1, D, H, W), dtype=torch.float32, device=grad_out.device)
    check(lib().m3d_conv3d_stem5_dgrad(_ptr(grad_out), _ptr(wf), _ptr(gin), B, Cc, D, H, W, _stream()), "conv3d_stem5_dgrad")
    return gin


def prm_scatter(windows, sums, origins, shape):
    _need_gpu(windows, sums, origins)
    P, Wn = windows.shape[0], windows.shape[1]
    D, H, W = shape
    dense = torch.empty((P, D, H, W), dtype=torch.float32, device=windows.device)     # the library writes every voxel
    check(lib().m3d_prm_scatter(_ptr(windows), _ptr(sums), _ptr(origins), P, Wn, D, H, W, _ptr(dense), _stream()), "prm_scatter")
    return dense


# ------------------------------------------------------------------ PRM post-processing -> Otsu
def prm_quantize_u8(prms):
    """prms float32 [P, D, H, W] CUDA -> uint8 [P, D, H, W] (infer_simple.py:233-238 per map)."""
    _need_gpu(prms)
    prms = _f32c(prms)
    out = torch.empty(prms.shape, dtype=torch.uint8, device=prms.device)
    P = prms.shape[0]
    check(lib().m3d_prm_quantize_u8(_ptr(prms), P, C.c_int64(prms[0].numel() if P else 1), _ptr(out), _stream()), "prm_quantize_u8")
    return out


def prm_quantize_windows_u8(windows, sums, origins, shape, return_nonempty=False):
    """The uint8 maps of prm_quantize_u8(prm_scatter(windows, sums, origins, shape)) without the dense float maps: windows
    float32 [P,Wn,Wn,Wn] (un-normalised, clamped), sums [P], origins int32 [P,3], shape = (D,H,W) -> uint8 [P,D,H,W]
    (+ bool [P]: the map has a non-zero voxel)."""
    _need_gpu(windows, sums, origins)
    windows = _f32c(windows)
    P, Wn = windows.shape[0], windows.shape[1]
    D, H, W = (int(v) for v in shape)
    out = torch.empty((P, D, H, W), dtype=torch.uint8, device=windows.device)
    ws = torch.empty((max(16 * P, 16),), dtype=torch.uint8, device=windows.device)
    check(lib().m3d_prm_quantize_windows_u8(_ptr(windows), _ptr(_f32c(sums)), _ptr(origins.contiguous()), P, Wn, D, H, W, _ptr(out),
                                            _ptr(ws), C.c_size_t(ws.numel()), _stream()), "prm_quantize_windows_u8")
    if return_nonempty:
        return out, ws[:16 * P].view(torch.int32).view(P, 4)[:, 3] != 0
    return out


def prm_quantize_windows_compact_u8(windows, sums, origins, shape, out=None, return_nonempty=False):
    """The uint8 values of prm_quantize_windows_u8 as windows [P,Wn,Wn,Wn] (0 outside the tile): with `origins`, everything a writer
    needs to rebuild each uint8 map (m3d.io.encode_window_stack_u8)."""
    _need_gpu(windows, sums, origins)
    windows = _f32c(windows)
    P, Wn = windows.shape[0], windows.shape[1]
    D, H, W = (int(v) for v in shape)
    _claim(out)
    if out is None:
        out = torch.empty((P, Wn, Wn, Wn), dtype=torch.uint8, device=windows.device)
    ws = torch.empty((max(16 * P, 16),), dtype=torch.uint8, device=windows.device)
    check(lib().m3d_prm_quantize_windows_compact_u8(_ptr(windows), _ptr(_f32c(sums)), _ptr(origins.contiguous()), P, Wn, D, H, W, _ptr(out),
                                                    _ptr(ws), C.c_size_t(ws.numel()), _stream()), "prm_quantize_windows_compact_u8")
    if return_nonempty == "stats":                   # the raw per-map words (word 3 != 0: the map has a non-zero voxel), for paint_begin
        return out, ws[:16 * P].view(torch.int32).view(P, 4)
    if return_nonempty:
        return out, ws[:16 * P].view(torch.int32).view(P, 4)[:, 3] != 0
    return out


def roi_normalize(image_u16, prm_u8, boxes, mode, boxes_host=None, map_index=None, win_origins=None, offsets=None):
    """image_u16 [D,H,W] uint16 CUDA; prm_u8 [R,D,H,W] uint8; boxes int32 [R,6] inclusive (x1,y1,z1,x2,y2,z2).
    Returns (img crops uint16 flat, prm crops uint16 flat, offsets int64 [R+1]) - the inputs of otsu2d_batch.
    boxes_host: the same boxes as an ndarray when the caller has them (saves the device read-back that sizes the crops).
    map_index (int32 [R] on the device): RoI r reads prm_u8[map_index[r]] - prm_u8 then holds ALL maps of the tile, not a gathered subset.
    win_origins (int32 [P,3]): prm_u8 is the COMPACT form [P,n,n,n] of prm_quantize_windows_compact_u8 (zero outside each window)."""
    _need_gpu(image_u16, prm_u8, boxes)
    assert image_u16.dtype == torch.uint16 and prm_u8.dtype == torch.uint8 and boxes.dtype == torch.int32
    R = boxes.shape[0]
    D, H, W = image_u16.shape
    win = 0 if win_origins is None else int(prm_u8.shape[1])
    if win_origins is not None:
        assert prm_u8.dim() == 4 and prm_u8.shape[1] == prm_u8.shape[2] == prm_u8.shape[3] and win_origins.dtype == torch.int32 and win_origins.is_contiguous()
    b = (np.asarray(boxes_host) if boxes_host is not None else boxes.cpu().numpy()).astype(np.int64)
    sizes = (b[:, 3] - b[:, 0] + 1) * (b[:, 4] - b[:, 1] + 1) * (b[:, 5] - b[:, 2] + 1)
    assert R == 0 or (sizes.min() > 0 and b[:, :3].min() >= 0 and b[:, 3].max() < W and b[:, 4].max() < H and b[:, 5].max() < D)
    offs_h = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    offs = upload(offs_h, image_u16.device) if offsets is None else offsets     # offsets: the caller uploaded crop_offsets(boxes_host) itself
    total = int(offs_h[-1]) if R else 0
    oi = torch.empty((total,), dtype=torch.uint16, device=image_u16.device)
    op = torch.empty((total,), dtype=torch.uint16, device=image_u16.device)
    if R == 0:
        return oi, op, offs
    ws = torch.empty((24 * R,), dtype=torch.uint8, device=image_u16.device)
    if map_index is not None:
        assert map_index.dtype == torch.int32 and map_index.is_cuda and map_index.numel() == R
    check(lib().m3d_roi_normalize_idx(_ptr(image_u16.contiguous()), _ptr(prm_u8.contiguous()), _ptr(map_index), win, _ptr(win_origins), _ptr(boxes.contiguous()), _ptr(offs),
                                     R, C.c_int64(total), D, H, W, {"soma": 0, "nuclei": 1}[mode], _ptr(oi), _ptr(op), _ptr(ws),
                                     C.c_size_t(ws.numel()), _stream()), "roi_normalize")
    return oi, op, offs


# ------------------------------------------------------------------ Winograd-x 3x3x3 forward
class _F16x2Conv3d(object):
    """What the two f16x2 3x3x3 conv wrappers share, over the entry-point family m3d_conv3d_<FAMILY>_* (ZwConv3d: "zw", ZnConv3d: "zn"):
    the weight packs (forward, and backward-data straight from the parameter's layout), the host queries, and how operand bounds
    travel.  The operand scale comes from a BOUND of the input's largest magnitude that travels with the activations: `in_max` is a
    device array of SLOTS floats (its largest entry is the bound; `bound_of(x)` sweeps a tensor), and every call returns the same kind of
    array for its OUTPUT (filled by the kernel's epilogue), so a chain of layers sweeps only its first input."""
    SLOTS = 32
    FAMILY = None

    @classmethod
    def _entry(cls, name):
        return getattr(lib(), "m3d_conv3d_%s_%s" % (cls.FAMILY, name))

    @classmethod
    def _takes(cls, cin, cout, D, H, W, pool):
        """m3d_conv3d_<FAMILY>_supported; only zw has a fused pool, and only its query takes the argument"""
        if cls.FAMILY == "zw":
            return bool(cls._entry("supported")(cin, cout, D, H, W, int(bool(pool))))
        return not pool and bool(cls._entry("supported")(cin, cout, D, H, W))

    @classmethod
    def supported(cls, weight, shape=None, pool=False):
        """weight [cout, cin, 3, 3, 3] with cin % 16 == 0; shape = (D, H, W) of the input (None: any supported map)."""
        if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or int(weight.shape[1]) % 16 != 0:
            return False
        if shape is None:
            return True
        D, H, W = (int(v) for v in shape)
        return cls._takes(int(weight.shape[1]), int(weight.shape[0]), D, H, W, pool)

    def _pack(self, w, cin, cout, entry):
        """the logical conv cin -> cout from the weight w [., ., 3, 3, 3], packed by m3d_conv3d_<FAMILY>_<entry>(w, w's cin, w's cout, ..)"""
        self.cout, self.cin = cout, cin
        nbytes = self._entry("packed_bytes")(cin, cout)
        self.packed = torch.empty((nbytes,), dtype=torch.uint8, device=w.device)
        check(self._entry(entry)(_ptr(w), int(w.shape[1]), int(w.shape[0]), _ptr(self.packed), _stream()), "conv3d_%s_%s" % (self.FAMILY, entry))

    def __init__(self, weight):
        _need_gpu(weight)
        w = _f32c(weight)
        assert self.supported(w)
        self._pack(w, int(w.shape[1]), int(w.shape[0]), "pack")

    @classmethod
    def dgrad_of(cls, weight):
        """The BACKWARD-DATA conv of a forward layer `weight` [cout, cin, 3, 3, 3] (cout % 16 == 0) as a conv of this class: cin = the
        layer's cout, cout = the layer's cin.  The pack comes straight from the parameter's own layout (m3d_conv3d_<FAMILY>_pack_dgrad):
        the bytes of cls(weight.flip(2, 3, 4).transpose(0, 1).contiguous()).packed without that copy."""
        cls._check_dgrad_weight(weight.dim() == 5 and tuple(weight.shape[2:]) == (3, 3, 3) and int(weight.shape[0]) % 16 == 0, weight)
        _need_gpu(weight)
        w = _f32c(weight)
        self = cls.__new__(cls)
        self._pack(w, int(w.shape[0]), int(w.shape[1]), "pack_dgrad")
        return self

    def supports(self, shape, pool=False):
        D, H, W = (int(v) for v in shape[-3:])
        return self._takes(self.cin, self.cout, D, H, W, pool)

    def units(self, shape):
        """workgroups of a launch on an input [B, cin, D, H, W] (or (D, H, W): one item): the library's own count, (64 channels) x (its tile)"""
        B = int(shape[0]) if len(shape) == 5 else 1
        D, H, W = (int(v) for v in shape[-3:])
        return int(self._entry("launch_units")(B, self.cin, self.cout, D, H, W))

    @staticmethod
    def bound_of(x):
        """[SLOTS] device floats, slot 0 = max |x| (one sweep of x)."""
        _need_gpu(x)
        x = _f32c(x)
        out = torch.empty((_F16x2Conv3d.SLOTS,), dtype=torch.float32, device=x.device)
        check(lib().m3d_conv3d_zw_bound_of(_ptr(x), C.c_longlong(x.numel()), _ptr(out), _stream()), "conv3d_zw_bound_of")
        return out

    def _operands(self, x, in_max, out, out_max, pool=False):
        """-> (x, out, out_max) of a launch: x contiguous fp32 [B, cin, D, H, W]; `out` claimed, or fresh; out_max: a ZEROED [SLOTS] float
        tensor to receive the output's bound (None: a fresh one; False: no bound output - the last layer of a chain - returned as None)"""
        _need_gpu(x, in_max)
        x = _f32c(x)
        B, cin, D, H, W = x.shape
        assert cin == self.cin and in_max.numel() == self.SLOTS and in_max.dtype == torch.float32
        oshape = (B, self.cout, D // 2, H // 2, W // 2) if pool else (B, self.cout, D, H, W)
        _claim(out)
        if out is None:
            out = torch.empty(oshape, dtype=torch.float32, device=x.device)
        assert tuple(out.shape) == oshape and out.is_contiguous()
        if out_max is None:
            out_max = torch.zeros((self.SLOTS,), dtype=torch.float32, device=x.device)
        elif out_max is False:
            out_max = None
        return x, out, out_max


class ZwConv3d(_F16x2Conv3d):
    """3x3x3 forward conv (stride 1, pad 1) + scale/shift + ReLU [+ MaxPool3d(2,2)] on the f16 matrix cores at fp32 accuracy
    (csrc/conv3d_zw.hip: f16x2 split, Winograd F(2,3) along z); operand bounds as _F16x2Conv3d says.  __call__ -> (out, out_max)."""
    FAMILY = "zw"

    @staticmethod
    def _check_dgrad_weight(ok, weight):
        assert ok

    def strip(self, gn, pitch, P, out=None, bounds=None):
        """PRM window strip gn [cin, planes, U, L] (windows side by side along x, cell p = columns [pitch p, pitch (p + 1)): strip_geometry
        mode 2) -> [cout, planes, U, L], one operand scale per window (bounds [P, 32], column 0 = the largest |value| of each window, e.g. what
        prm_prepare(peak_max=True) left on gn; None: swept here, m3d_prm_strip_absmax).  Returns None when the library has no
        configuration for the shape."""
        _need_gpu(gn)
        assert gn.dim() == 4 and gn.shape[0] == self.cin and gn.is_contiguous() and gn.dtype == torch.float32
        cin, D, H, L = (int(v) for v in gn.shape)
        if L < 24 or not self.supports((D, H, L)) or gn.numel() * 4 >= 0x7FFFFF00 or pitch % 4 or L % 4:
            return None
        bounds = self._strip_bounds(gn, pitch, P, bounds)
        if bounds is None:
            return None
        _claim(out)
        if out is None:
            out = torch.empty((self.cout, D, H, L), dtype=torch.float32, device=gn.device)
        check(lib().m3d_conv3d_zw_forward_strip(_ptr(gn), _ptr(self.packed), _ptr(out), cin, self.cout, D, H, L, _ptr(bounds), int(P), int(pitch),
                                                _stream()), "conv3d_zw_forward_strip")
        return out

    STRIP_SWEEP_MAX_PEAKS = 12288                           # windows one m3d_prm_strip_absmax sweep takes (one LDS float per window)

    def _strip_bounds(self, gn, pitch, P, bounds):
        """the per-window operand bounds [P, 32] of a strip conv, or None where they are not given and the strip has more windows than
        the sweep takes (the caller then returns None: the fp32 strip kernels run instead)"""
        if bounds is None and P > self.STRIP_SWEEP_MAX_PEAKS:
            return None
        if bounds is None:                                  # (the producer did not leave them: one sweep of the strip)
            bounds = torch.empty((P, 32), dtype=torch.float32, device=gn.device)
            check(lib().m3d_prm_strip_absmax(_ptr(gn), C.c_longlong(gn.shape[0] * gn.shape[1] * gn.shape[2]), int(gn.shape[3]), int(pitch), int(P),
                                             _ptr(bounds), _stream()), "prm_strip_absmax")
        assert tuple(bounds.shape) == (P, 32) and bounds.dtype == torch.float32 and bounds.is_contiguous()
        return bounds

    def strip_prepare(self, gn, dims, origin, xnext, scale, norm, up_off, in_slab=False, out_slab=False, bounds=None):
        """WinoConv3d.strip_prepare on this kernel (m3d_prm_strip_dgrad_prepare_zw): the strip conv fused with the prepare step of the layer
        below; (strip [cout, planes', U + 2, L(U + 2)], origin - 1), or None where the library has no configuration."""
        _need_gpu(gn, origin, xnext, norm, up_off)
        P, cin, U = (int(v) for v in dims)
        assert cin == self.cin and xnext.shape[0] == self.cout == norm.shape[0] and xnext.shape == norm.shape
        MD, MH, MW = (int(v) for v in norm.shape[1:])
        in_slab, out_slab = bool(in_slab), bool(out_slab)
        pitch, _, L = strip_geometry(U, 2, P)
        assert tuple(gn.shape) == (cin, MD if in_slab else U, U, L) and gn.is_contiguous()
        if L < 24 or pitch % 4 or gn.numel() * 4 >= 0x7FFFFF00 or not self.supports((gn.shape[1], U, L)):
            return None
        bounds = self._strip_bounds(gn, pitch, P, bounds)
        if bounds is None:
            return None
        out = torch.empty((self.cout, MD if out_slab else U + 2, U + 2, strip_geometry(U + 2, 2, P)[2]), dtype=torch.float32, device=gn.device)
        oo = torch.empty((P, 3), dtype=torch.int32, device=gn.device)
        rc = lib().m3d_prm_strip_dgrad_prepare_zw(_ptr(gn), _ptr(self.packed), cin, self.cout, P, U, int(in_slab), _ptr(origin), _ptr(xnext),
                                                  _ptr(norm), _ptr(scale), _ptr(up_off), MD, MH, MW, int(out_slab), _ptr(bounds), _ptr(out),
                                                  _ptr(oo), _stream())
        if rc == -4:                                        # M3D_EUNSUPPORTED
            return None
        check(rc, "prm_strip_dgrad_prepare_zw")
        return out, oo

    def __call__(self, x, in_max, scale=None, shift=None, relu=False, pool=False, out=None, out_max=None):
        """out_max: a ZEROED [SLOTS] float tensor to receive the output's bound (None: a fresh one; False: no bound output)."""
        x, out, out_max = self._operands(x, in_max, out, out_max, pool=pool)
        assert x[0].numel() * 4 < 0x7FFFFFFF                  # one batch item is addressed with 32-bit buffer offsets
        B, cin, D, H, W = x.shape
        check(lib().m3d_conv3d_zw_forward(_ptr(x), _ptr(self.packed), _ptr(out), B, cin, self.cout, D, H, W,
                                          _ptr(scale) if scale is not None else None, _ptr(shift) if shift is not None else None,
                                          int(bool(relu)), int(bool(pool)), _ptr(in_max), _ptr(out_max) if out_max is not None else None,
                                          _stream()), "conv3d_zw_forward")
        return out, out_max


class ZnConv3d(_F16x2Conv3d):
    """3x3x3 conv (stride 1, padding = dilation, dilation 1 or 2) + scale/shift + ReLU on maps at most 8 wide - the per-RoI convs on 7^3
    RoI grids - on the f16 matrix cores at fp32 accuracy (csrc/conv3d_zn.hip: f16x2 split, direct 27 taps, one workgroup per 64 channels
    x 8 x 8 x 4 voxels, no atomics on the output); operand bounds as _F16x2Conv3d says (bound_of is ZwConv3d's sweep).  No fused pool.
    __call__ -> (out, out_max).  A pack serves both dilations (ZnConv3d(weight) and dgrad_of(weight) alike): dilation 1 takes
    m3d_conv3d_zn_forward and the queries beside it, exactly as before the argument existed; dilation 2 (the mask head at
    MRCNN.DILATION = 2) takes m3d_conv3d_zn_dilated_forward / _supported / _launch_units."""
    FAMILY = "zn"

    @staticmethod
    def _check_dgrad_weight(ok, weight):
        if not ok:
            raise ValueError("ZnConv3d.dgrad_of: weight [cout, cin, 3, 3, 3] with cout %% 16 == 0, got %s" % (tuple(weight.shape),))

    def supports(self, shape, pool=False, dilation=1):
        if int(dilation) == 1:
            return super().supports(shape, pool)
        D, H, W = (int(v) for v in shape[-3:])
        return not pool and bool(lib().m3d_conv3d_zn_dilated_supported(self.cin, self.cout, D, H, W, int(dilation)))

    def units(self, shape, dilation=1):
        if int(dilation) == 1:
            return super().units(shape)
        B = int(shape[0]) if len(shape) == 5 else 1
        D, H, W = (int(v) for v in shape[-3:])
        return int(lib().m3d_conv3d_zn_dilated_launch_units(B, self.cin, self.cout, D, H, W, int(dilation)))

    def __call__(self, x, in_max, scale=None, shift=None, relu=False, out=None, out_max=None, dilation=1):
        """out_max: a ZEROED [SLOTS] float tensor to receive the output's bound (None: a fresh one; False: no bound output)."""
        x, out, out_max = self._operands(x, in_max, out, out_max)
        B, cin, D, H, W = x.shape
        if int(dilation) != 1:
            check(lib().m3d_conv3d_zn_dilated_forward(_ptr(x), _ptr(self.packed), _ptr(out), B, cin, self.cout, D, H, W, int(dilation),
                                                      _ptr(scale) if scale is not None else None, _ptr(shift) if shift is not None else None,
                                                      int(bool(relu)), _ptr(in_max), _ptr(out_max) if out_max is not None else None,
                                                      _stream()), "conv3d_zn_dilated_forward")
            return out, out_max
        check(lib().m3d_conv3d_zn_forward(_ptr(x), _ptr(self.packed), _ptr(out), B, cin, self.cout, D, H, W,
                                          _ptr(scale) if scale is not None else None, _ptr(shift) if shift is not None else None,
                                          int(bool(relu)), _ptr(in_max), _ptr(out_max) if out_max is not None else None,
                                          _stream()), "conv3d_zn_forward")
        return out, out_max


class WinoConv3d(object):
    """3x3x3 forward conv (stride 1, pad 1) through a Winograd MFMA kernel; weights transformed and packed once.
    two_d=False: F(2,3) along x (2/3 of the MFMA work); two_d=True: F(2x2,3x3) on the (y,x) plane (4/9).
    `supports(width)` says whether the kernel has a tile configuration for the map (else use PackedConv3d)."""

    def __init__(self, weight, two_d=False, local=False):
        """local=True (2-D kernels): only the F(2x2,3x3) family, whose outputs depend on nothing outside their own 3 x 3 support even by
        rounding - for data laid out with unrelated neighbours (the PRM strips); the default family uses F(4,3) along x."""
        _need_gpu(weight)
        w = _f32c(weight)
        assert w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3)
        self.cout, self.cin = int(w.shape[0]), int(w.shape[1])
        self.two_d = bool(two_d)
        self.local = bool(local) and self.two_d
        L = lib()
        self._bytes, self._pack, self._fwd, self._pool = \
            (L.m3d_conv3d_wino2_packed_weight_bytes, L.m3d_conv3d_wino2_pack_weights, L.m3d_conv3d_wino2_forward,
             L.m3d_conv3d_wino2_forward_pool2) if self.two_d else \
            (L.m3d_conv3d_wino_packed_weight_bytes, L.m3d_conv3d_wino_pack_weights, L.m3d_conv3d_wino_forward,
             L.m3d_conv3d_wino_forward_pool2)
        nbytes = self._bytes(self.cin, self.cout)
        self.packed = torch.empty((nbytes // 4,), dtype=torch.float32, device=w.device)
        check(self._pack(_ptr(w), self.cin, self.cout, _ptr(self.packed), _stream()), "wino_pack")

    def supports(self, width, shape=None):
        """maps >= 24 voxels wide; the 2-D kernel also has a 16-wide tile with split-K from 12.  With shape = (B, D, H, W)
        the 2-D kernel additionally asks the library whether its tiles fit the map well enough to beat the direct kernel."""
        if width < (12 if self.two_d else 24):
            return False
        if self.two_d and shape is not None:
            B, D, H, W = (int(v) for v in shape)
            # below ~0.3 of useful tile volume x chip fill the direct kernel wins (tools/bench_wino_threshold.py; with F(2x4,3x3) the
            # 0.39-score layers of the soma net run 0.194 vs 0.253 ms, so the round-2 threshold of 0.5 came down)
            score = lib().m3d_conv3d_wino2_local_score if self.local else lib().m3d_conv3d_wino2_score     # each family asks about its own tiles
            return score(B, self.cin, self.cout, D, H, W) >= 0.3
        return True

    def __call__(self, x, scale=None, shift=None, relu=False, out=None):
        _need_gpu(x)
        x = _f32c(x)
        B, cin, D, H, W = x.shape
        assert cin == self.cin
        _claim(out)
        if out is None:
            out = torch.empty((B, self.cout, D, H, W), dtype=torch.float32, device=x.device)
        if self.two_d:                                     # the library picks the tile; small / ragged maps may split K
            wsb_fn, fwd_fn = (lib().m3d_conv3d_wino2_local_workspace_bytes, lib().m3d_conv3d_wino2_local_forward_ws) if self.local else \
                             (lib().m3d_conv3d_wino2_workspace_bytes, lib().m3d_conv3d_wino2_forward_ws)
            wsb = wsb_fn(B, cin, self.cout, D, H, W)
            key = (torch.cuda.current_stream().cuda_stream, x.device)           # one scratch buffer per stream: tiles on
            cache = self.__dict__.setdefault("_ws", {})                           # different streams run concurrently
            ws = cache.get(key)
            if ws is None or ws.numel() < wsb:
                ws = cache[key] = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=x.device)
            check(fwd_fn(_ptr(x), _ptr(self.packed), _ptr(out), B, cin, self.cout, D, H, W,
                         _ptr(scale) if scale is not None else None,
                         _ptr(shift) if shift is not None else None, int(bool(relu)),
                         _ptr(ws), C.c_size_t(wsb), _stream()), "conv3d_wino2_forward_ws")
            return out
        check(self._fwd(_ptr(x), _ptr(self.packed), _ptr(out), B, cin, self.cout, D, H, W,
                        _ptr(scale) if scale is not None else None, _ptr(shift) if shift is not None else None,
                        int(bool(relu)), _stream()), "conv3d_wino_forward")
        return out

    def plan(self, shape):
        """(family, tile id, K split) the library would use for an input [B, cin, D, H, W] (m3d_conv3d_wino2_plan; 2-D kernels only)."""
        B, D, H, W = (int(shape[0]),) + tuple(int(v) for v in shape[-3:])
        f, t, k = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().m3d_conv3d_wino2_plan(int(self.local), B, self.cin, self.cout, D, H, W, C.byref(f), C.byref(t), C.byref(k)), "conv3d_wino2_plan")
        return f.value, t.value, k.value

    def strip_prepare(self, gn, dims, origin, xnext, scale, norm, up_off, in_slab=False, out_slab=False):
        """PRM strips: this conv's backward-data on the prepared strip `gn` [cin, planes, U, L(U)] (quad-aligned layout, dims = (P, cin, U))
        FUSED with the prepare step of the layer below (xnext / scale / norm / up_off as ops.prm_prepare with pool = False, border = 1):
        returns (strip [cout, planes', U + 2, L(U + 2)], origin - 1), exactly what prm_prepare(out_strip=2) would make of this conv's
        result - or None when the library runs this shape through another kernel (the caller then takes the two launches)."""
        _need_gpu(gn, origin, xnext, norm, up_off)
        assert self.two_d and not self.local
        P, cin, U = (int(v) for v in dims)
        assert cin == self.cin and xnext.shape[0] == self.cout == norm.shape[0] and xnext.shape == norm.shape
        MD, MH, MW = (int(v) for v in norm.shape[1:])
        in_slab, out_slab = bool(in_slab), bool(out_slab)
        assert tuple(gn.shape) == (cin, MD if in_slab else U, U, strip_geometry(U, 2, P)[2]) and gn.is_contiguous()
        out = torch.empty((self.cout, MD if out_slab else U + 2, U + 2, strip_geometry(U + 2, 2, P)[2]), dtype=torch.float32, device=gn.device)
        oo = torch.empty((P, 3), dtype=torch.int32, device=gn.device)
        rc = lib().m3d_prm_strip_dgrad_prepare(_ptr(gn), _ptr(self.packed), cin, self.cout, P, U, int(in_slab), _ptr(origin), _ptr(xnext), _ptr(norm),
                                               _ptr(scale), _ptr(up_off), MD, MH, MW, int(out_slab), _ptr(out), _ptr(oo), _stream())
        if rc == -4:                                        # M3D_EUNSUPPORTED
            return None
        check(rc, "prm_strip_dgrad_prepare")
        return out, oo

    def supports_pool(self, width):
        return width >= (24 if self.two_d else 48)

    def pooled(self, x, scale=None, shift=None, relu=False, out=None, return_argmax=False):
        """conv + scale/shift + ReLU + MaxPool3d(2,2) in one launch; returns [B,cout,D//2,H//2,W//2] (+ the pool's uint8 argmax,
        2-D kernel only)."""
        _need_gpu(x)
        x = _f32c(x)
        B, cin, D, H, W = x.shape
        assert cin == self.cin
        _claim(out)
        if out is None:
            out = torch.empty((B, self.cout, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
        if return_argmax:
            assert self.two_d
            am = torch.empty(out.shape, dtype=torch.uint8, device=x.device)
            check(lib().m3d_conv3d_wino2_forward_pool2_argmax(_ptr(x), _ptr(self.packed), _ptr(out), _ptr(am), B, cin, self.cout, D, H, W,
                                                              _ptr(scale) if scale is not None else None,
                                                              _ptr(shift) if shift is not None else None, int(bool(relu)), _stream()),
                  "conv3d_wino2_forward_pool2_argmax")
            return out, am
        check(self._pool(_ptr(x), _ptr(self.packed), _ptr(out), B, cin, self.cout, D, H, W,
                         _ptr(scale) if scale is not None else None,
                         _ptr(shift) if shift is not None else None, int(bool(relu)), _stream()),
              "conv3d_wino_forward_pool2")
        return out


def conv3d_wino2_plan(batch, cin, cout, depth, height, width, local=False):
    """(family, tile id, K split) of the 2-D Winograd launch for this shape (m3d_conv3d_wino2_plan, host only): what WinoConv3d(two_d=True,
    local=local) runs."""
    f, t, k = C.c_int(0), C.c_int(0), C.c_int(0)
    check(lib().m3d_conv3d_wino2_plan(int(bool(local)), int(batch), int(cin), int(cout), int(depth), int(height), int(width), C.byref(f),
                                      C.byref(t), C.byref(k)), "conv3d_wino2_plan")
    return f.value, t.value, k.value


def conv3d_stem_wino_plan(batch, cout, depth, height, width, pool=False):
    """planes per workgroup (4 / 8) of the stem's rows kernel for this shape (m3d_conv3d_stem_wino_plan, host only), or None where the
    launch would return M3D_EUNSUPPORTED"""
    p = C.c_int(-1)
    rc = lib().m3d_conv3d_stem_wino_plan(int(batch), int(cout), int(depth), int(height), int(width), int(bool(pool)), C.byref(p))
    if rc == -4:                                            # M3D_EUNSUPPORTED
        return None
    check(rc, "conv3d_stem_wino_plan")
    return p.value


class StemWinoConv3d(object):
    """conv1a (5x5x5, Cin = 1, stride 1, pad 2) through the Winograd F(2,5)-along-x MFMA kernel, optionally fused with
    MaxPool3d(2,2); maps >= 32 voxels wide (else use PackedConv3d)."""

    def __init__(self, weight):
        _need_gpu(weight)
        w = _f32c(weight)
        assert w.dim() == 5 and tuple(w.shape[1:]) == (1, 5, 5, 5)
        self.cout, self.cin = int(w.shape[0]), 1
        nbytes = lib().m3d_conv3d_stem_wino_packed_weight_bytes(self.cout)
        self.packed = torch.empty((nbytes // 4,), dtype=torch.float32, device=w.device)
        check(lib().m3d_conv3d_stem_wino_pack_weights(_ptr(w), self.cout, _ptr(self.packed), _stream()), "stem_wino_pack")

    @staticmethod
    def supports(width):
        return width >= 32

    def plan(self, shape, pool=False):
        """planes per workgroup (4 / 8) of the kernel the library would launch for an input [B, 1, D, H, W] (m3d_conv3d_stem_wino_plan,
        host only) - or None where the launch would return M3D_EUNSUPPORTED"""
        return conv3d_stem_wino_plan(int(shape[0]), self.cout, *(int(v) for v in shape[-3:]), pool=pool)

    def _run(self, x, scale, shift, relu, pool, out, bound=False):
        _need_gpu(x)
        x = _f32c(x)
        B, cin, D, H, W = x.shape
        assert cin == 1
        _claim(out)
        if out is None:
            shp = (B, self.cout, D // 2, H // 2, W // 2) if pool else (B, self.cout, D, H, W)
            out = torch.empty(shp, dtype=torch.float32, device=x.device)
        # bound: False / None, or a ZEROED [ZwConv3d.SLOTS] float tensor of the caller's that the epilogue fills with the output's operand bound
        om = None if bound is False else bound
        check(lib().m3d_conv3d_stem_wino_forward_bound(_ptr(x), _ptr(self.packed), _ptr(out), B, self.cout, D, H, W,
                                                       _ptr(scale) if scale is not None else None,
                                                       _ptr(shift) if shift is not None else None, int(bool(relu)), int(bool(pool)),
                                                       _ptr(om) if om is not None else None, _stream()), "conv3d_stem_wino_forward")
        return out

    def __call__(self, x, scale=None, shift=None, relu=False, out=None, bound=False):
        return self._run(x, scale, shift, relu, False, out, bound)

    def pooled(self, x, scale=None, shift=None, relu=False, bound=False):
        return self._run(x, scale, shift, relu, True, None, bound)


# ------------------------------------------------------------------ conv backward-weights / bias gradient
def _wgrad_operands(x, grad_out, k, *bounds):
    """What every conv3d_wgrad* begins with: x [B,cin,D,H,W] and grad_out [B,cout,D,H,W] (and the bounds, where given) are CUDA tensors;
    -> (x, grad_out) as contiguous fp32, the dW [cout,cin,k,k,k] to fill, (B, cin, cout, D, H, W)"""
    _need_gpu(x, grad_out, *bounds)
    x, grad_out = _f32c(x), _f32c(grad_out)
    B, cin, D, H, W = x.shape
    cout = grad_out.shape[1]
    assert grad_out.shape == (B, cout, D, H, W)
    return x, grad_out, torch.empty((cout, cin, k, k, k), dtype=torch.float32, device=x.device), (B, cin, cout, D, H, W)


def _wgrad_f16_bounds(x, grad_out, x_max, gy_max):
    """(x_max, gy_max) of an f16x2 weight gradient: a missing one is swept (ZwConv3d.bound_of); each is [ZwConv3d.SLOTS] fp32"""
    if x_max is None:
        x_max = ZwConv3d.bound_of(x)
    if gy_max is None:
        gy_max = ZwConv3d.bound_of(grad_out)
    assert x_max.numel() == ZwConv3d.SLOTS and gy_max.numel() == ZwConv3d.SLOTS and x_max.dtype == gy_max.dtype == torch.float32
    return x_max, gy_max


def _wgrad_plan(entry, keys, *args):
    """A host-only m3d_<entry> with one int out-parameter per key after `args` -> dict(key: value)"""
    v = [C.c_int(0) for _ in keys]
    check(getattr(lib(), "m3d_" + entry)(*[int(a) for a in args], *[C.byref(a) for a in v]), entry)
    return dict(zip(keys, (a.value for a in v)))


def conv3d_wgrad_dilated_plan(batch, cin, cout, D, H, W, tile_x=0):
    """What conv3d_wgrad(..., 3, dilation=2) launches for this shape (m3d_conv3d_wgrad_dilated_plan, host only): dict(tile_x, tile_y, slots);
    tile_x = 16 / 8 asks for that tile form instead of the library's choice."""
    return _wgrad_plan("conv3d_wgrad_dilated_plan", ("tile_x", "tile_y", "slots"), batch, cin, cout, D, H, W, 3, 2, tile_x)


def conv3d_wgrad(x, grad_out, k, dilation=1, tile_x=0):
    """dW [cout,cin,k,k,k] of a stride-1 conv with padding dilation * (k // 2): x [B,cin,D,H,W], grad_out [B,cout,D,H,W] (fp32 CUDA).
    dilation 1 is m3d_conv3d_wgrad; k = 3 with dilation 2 is m3d_conv3d_wgrad_dilated (tile_x = 16 / 8: that voxel tile instead of the
    library's choice, for A/B runs and tests); any other dilation is an error."""
    x, grad_out, dw, shape = _wgrad_operands(x, grad_out, k)
    if dilation != 1:
        wsb = lib().m3d_conv3d_wgrad_dilated_workspace_bytes(*shape, k, int(dilation))
        ws = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=x.device)
        if tile_x:
            rc = lib().m3d_conv3d_wgrad_dilated_tile(_ptr(x), _ptr(grad_out), _ptr(dw), *shape, k, int(dilation), int(tile_x), _ptr(ws),
                                                     C.c_size_t(wsb), _stream())
        else:
            rc = lib().m3d_conv3d_wgrad_dilated(_ptr(x), _ptr(grad_out), _ptr(dw), *shape, k, int(dilation), _ptr(ws), C.c_size_t(wsb),
                                                _stream())
        check(rc, "conv3d_wgrad_dilated")
        return dw
    wsb = lib().m3d_conv3d_wgrad_workspace_bytes(*shape, k)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=x.device)
    check(lib().m3d_conv3d_wgrad(_ptr(x), _ptr(grad_out), _ptr(dw), *shape, k, _ptr(ws), C.c_size_t(wsb), _stream()), "conv3d_wgrad")
    return dw


def conv3d_wgrad_narrow_supported(batch, cin, cout, D, H, W, k=3):
    """m3d_conv3d_wgrad_narrow_supported (host only): the dilation-1 weight gradient of this shape runs on the 2 x 8 x 8 tile kernel
    (k = 3, W <= 8)"""
    return bool(lib().m3d_conv3d_wgrad_narrow_supported(int(batch), int(cin), int(cout), int(D), int(H), int(W), int(k)))


def conv3d_wgrad_narrow_plan(batch, cin, cout, D, H, W):
    """What conv3d_wgrad_narrow launches for this shape (m3d_conv3d_wgrad_narrow_plan, host only): dict(tile_x, tile_y, slots)"""
    return _wgrad_plan("conv3d_wgrad_narrow_plan", ("tile_x", "tile_y", "slots"), batch, cin, cout, D, H, W, 3)


def conv3d_wgrad_narrow(x, grad_out):
    """dW [cout,cin,3,3,3] of a stride-1 pad-1 3^3 conv on a map at most 8 wide (m3d_conv3d_wgrad_narrow: fp32 MFMA on the 2 x 8 x 8
    voxel tile): x [B,cin,D,H,W], grad_out [B,cout,D,H,W] (fp32 CUDA).  An unsupported shape is an error: ask
    conv3d_wgrad_narrow_supported (or conv_plan.wgrad_kernel)."""
    x, grad_out, dw, shape = _wgrad_operands(x, grad_out, 3)
    wsb = lib().m3d_conv3d_wgrad_narrow_workspace_bytes(*shape, 3)
    ws = torch.empty((max(wsb, 1),), dtype=torch.uint8, device=x.device)
    check(lib().m3d_conv3d_wgrad_narrow(_ptr(x), _ptr(grad_out), _ptr(dw), *shape, 3, _ptr(ws), C.c_size_t(wsb), _stream()),
          "conv3d_wgrad_narrow")
    return dw


def conv3d_wgrad_f16x2_supported(batch, cin, cout, D, H, W):
    """m3d_conv3d_wgrad_f16x2_supported (host only): the k = 3 weight gradient of this shape runs on the f16 matrix cores"""
    return bool(lib().m3d_conv3d_wgrad_f16x2_supported(int(batch), int(cin), int(cout), int(D), int(H), int(W)))


def conv3d_wgrad_f16x2_plan(batch, cin, cout, D, H, W):
    """The host decision of the launch (m3d_conv3d_wgrad_f16x2_plan): dict(slots, tiles_per_slot, chain, folds)"""
    return _wgrad_plan("conv3d_wgrad_f16x2_plan", ("slots", "tiles_per_slot", "chain", "folds"), batch, cin, cout, D, H, W)


def conv3d_wgrad_f16x2(x, grad_out, x_max=None, gy_max=None):
    """dW [cout,cin,3,3,3] of a stride-1 pad-1 3^3 conv on the f16 matrix cores at fp32 accuracy (m3d_conv3d_wgrad_f16x2): x [B,cin,D,H,W],
    grad_out [B,cout,D,H,W] (fp32 CUDA).  x_max / gy_max: [ZwConv3d.SLOTS] device floats whose largest bounds |x| / |grad_out|; a missing
    one is swept (ZwConv3d.bound_of).  An unsupported shape is an error: ask conv3d_wgrad_f16x2_supported (or conv_plan.wgrad_kernel)."""
    x, grad_out, dw, shape = _wgrad_operands(x, grad_out, 3, x_max, gy_max)
    x_max, gy_max = _wgrad_f16_bounds(x, grad_out, x_max, gy_max)
    wsb = lib().m3d_conv3d_wgrad_f16x2_workspace_bytes(*shape)
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=x.device)
    check(lib().m3d_conv3d_wgrad_f16x2(_ptr(x), _ptr(grad_out), _ptr(dw), *shape, _ptr(x_max), _ptr(gy_max), _ptr(ws), C.c_size_t(wsb),
                                       _stream()), "conv3d_wgrad_f16x2")
    return dw


# The three narrow f16x2 wrappers below call the dilation-1 entry points when `dilation` is 1 and the ones that take the dilation
# otherwise, although the former only forward to the latter: the launch records of tests/test_wgrad_dilated_f16_host.py and
# tests/test_conv_train_dispatch_narrow_f16.py pin which symbol a dilation-1 call reaches.
def conv3d_wgrad_narrow_f16x2_supported(batch, cin, cout, D, H, W, dilation=1):
    """m3d_conv3d_wgrad_narrow_f16x2_supported (host only): the k = 3 weight gradient of this shape runs on the f16 matrix cores on the
    2 x 8 x 8 voxel tile (W <= 8, cin and cout multiples of 32).  dilation: 1 (left out: that query) or another one, asked of
    m3d_conv3d_wgrad_narrow_dilated_f16x2_supported (which takes 1 and 2)"""
    if dilation == 1:
        return bool(lib().m3d_conv3d_wgrad_narrow_f16x2_supported(int(batch), int(cin), int(cout), int(D), int(H), int(W)))
    return bool(lib().m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(int(batch), int(cin), int(cout), int(D), int(H), int(W), int(dilation)))


def conv3d_wgrad_narrow_f16x2_plan(batch, cin, cout, D, H, W, dilation=1):
    """The host decision of the launch (m3d_conv3d_wgrad_narrow_f16x2_plan; with a dilation other than 1
    m3d_conv3d_wgrad_narrow_dilated_f16x2_plan): dict(tile_z, slots, tiles_per_slot, chain, folds)"""
    keys = ("tile_z", "slots", "tiles_per_slot", "chain", "folds")
    if dilation == 1:
        return _wgrad_plan("conv3d_wgrad_narrow_f16x2_plan", keys, batch, cin, cout, D, H, W)
    return _wgrad_plan("conv3d_wgrad_narrow_dilated_f16x2_plan", keys, batch, cin, cout, D, H, W, dilation)


def conv3d_wgrad_narrow_f16x2(x, grad_out, x_max=None, gy_max=None, dilation=1):
    """conv3d_wgrad_f16x2 for maps at most 8 wide (m3d_conv3d_wgrad_narrow_f16x2: the same cut on the 2 x 8 x 8 voxel tile): x
    [B,cin,D,H,W], grad_out [B,cout,D,H,W] (fp32 CUDA) -> dW [cout,cin,3,3,3].  x_max / gy_max: [ZwConv3d.SLOTS] device floats whose
    largest bounds |x| / |grad_out|; a missing one is swept (ZwConv3d.bound_of).  dilation: 1 (left out: the calls above), or 2: the
    weight gradient of the dilation-2, padding-2 conv (m3d_conv3d_wgrad_narrow_dilated_f16x2).  An unsupported shape or dilation is an
    error: ask conv3d_wgrad_narrow_f16x2_supported (or conv_plan.plan_train_conv)."""
    x, grad_out, dw, shape = _wgrad_operands(x, grad_out, 3, x_max, gy_max)
    x_max, gy_max = _wgrad_f16_bounds(x, grad_out, x_max, gy_max)
    name, dil = ("conv3d_wgrad_narrow_f16x2", ()) if dilation == 1 else ("conv3d_wgrad_narrow_dilated_f16x2", (int(dilation),))
    wsb = getattr(lib(), "m3d_%s_workspace_bytes" % name)(*shape, *dil)
    ws = torch.empty((max(wsb, 16),), dtype=torch.uint8, device=x.device)
    check(getattr(lib(), "m3d_" + name)(_ptr(x), _ptr(grad_out), _ptr(dw), *shape, *dil, _ptr(x_max), _ptr(gy_max), _ptr(ws),
                                        C.c_size_t(wsb), _stream()), name)
    return dw


def conv3d_bias_grad(grad_out):
    _need_gpu(grad_out)
    grad_out = _f32c(grad_out)
    B, cout, D, H, W = grad_out.shape
    db = torch.empty((cout,), dtype=torch.float32, device=grad_out.device)
    check(lib().m3d_conv3d_bias_grad(_ptr(grad_out), _ptr(db), B, cout, D, H, W, _stream()), "conv3d_bias_grad")
    return db


def conv3d_gy_reduce(grad_out, bias=True):
    """(gb or None, gy_max) from ONE pass over grad_out [B, cout, D, H, W] (m3d_conv3d_gy_reduce): gb [cout] = fp32 of the fp64 sum over
    (B, D, H, W) (fixed order: bit-identical run to run), gy_max [ZwConv3d.SLOTS] device floats whose largest is max |grad_out| exactly -
    the operand bound ZwConv3d.dgrad_of(w)(grad_out, gy_max) and conv3d_wgrad_f16x2(.., gy_max=) take.  No host read."""
    _need_gpu(grad_out)
    grad_out = _f32c(grad_out)
    B, cout, D, H, W = (int(v) for v in grad_out.shape)
    gb = torch.empty((cout,), dtype=torch.float32, device=grad_out.device) if bias else None
    gy_max = torch.empty((ZwConv3d.SLOTS,), dtype=torch.float32, device=grad_out.device)
    wsb = C.c_size_t(0)
    check(lib().m3d_conv3d_gy_reduce(None, B, cout, D, H, W, None, None, None, C.byref(wsb), None), "conv3d_gy_reduce")
    ws = torch.empty((max(wsb.value, 8),), dtype=torch.uint8, device=grad_out.device)
    wsb = C.c_size_t(ws.numel())
    check(lib().m3d_conv3d_gy_reduce(_ptr(grad_out), B, cout, D, H, W, _ptr(gb) if bias else None, _ptr(gy_max), _ptr(ws), C.byref(wsb),
                                     _stream()), "conv3d_gy_reduce")
    return gb, gy_max


# ------------------------------------------------------------------ volume pre-filters (binarization_nuclei.py:44-45)
def gaussian_filter_u16(vol, sigma=1.0, truncate=4.0):
    """scipy.ndimage.gaussian_filter(vol, sigma) for a uint16 CUDA volume [D,H,W], bit-exact (uint16 after every pass)."""
    _need_gpu(vol)
    assert vol.dtype == torch.uint16 and vol.dim() == 3
    vol = vol.contiguous()
    radius = int(truncate * float(sigma) + 0.5)                      # scipy/ndimage/_filters.py gaussian_filter1d
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2)      # _gaussian_kernel1d, order 0
    phi = phi / phi.sum()
    w = torch.from_numpy(np.ascontiguousarray(phi[radius:])).to(vol.device)      # centre first
    out, tmp = torch.empty_like(vol), torch.empty_like(vol)
    D, H, W = vol.shape
    check(lib().m3d_gaussian_filter_u16(_ptr(vol), _ptr(out), _ptr(tmp), D, H, W, _ptr(w), radius, _stream()), "gaussian_filter_u16")
    return out


def median_filter3_u16(vol):
    """scipy.ndimage.median_filter(vol, size=3) for a uint16 CUDA volume [D,H,W]."""
    _need_gpu(vol)
    assert vol.dtype == torch.uint16 and vol.dim() == 3
    vol = vol.contiguous()
    out = torch.empty_like(vol)
    D, H, W = vol.shape
    check(lib().m3d_median_filter3_u16(_ptr(vol), _ptr(out), D, H, W, _stream()), "median_filter3_u16")
    return out


# ------------------------------------------------------------------ connected components / closing / painting
def cc_largest_batch(mask, offsets, dims, invert=False, tie_last=True):
    """mask uint8 flat (crops concatenated), offsets int64 [R+1], dims int32 [R,3] (ez,ey,ex).
    Returns (out uint8 flat {0,255}, status int32 [R])."""
    _need_gpu(mask, offsets, dims)
    assert mask.dtype == torch.uint8 and offsets.dtype == torch.int64 and dims.dtype == torch.int32
    R = dims.shape[0]
    total = int(mask.numel())
    out = torch.empty_like(mask)
    status = torch.empty((R,), dtype=torch.int32, device=mask.device)        # cc_init (bad crop: 2) / cc_write (0 / 1) write every entry
    wsb = lib().m3d_cc_workspace_bytes(C.c_int64(total))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=mask.device)
    check(lib().m3d_cc_largest_batch(_ptr(mask), _ptr(offsets), _ptr(dims.contiguous()), R, C.c_int64(total), int(bool(invert)),
                                     int(bool(tie_last)), _ptr(out), _ptr(status), _ptr(ws), C.c_size_t(wsb), _stream()),
          "cc_largest_batch")
    return out, status


def binary_closing6_batch(mask, offsets, dims):
    _need_gpu(mask, offsets, dims)
    R = dims.shape[0]
    total = int(mask.numel())
    out = torch.empty_like(mask)
    ws = torch.empty((total + 512,), dtype=torch.uint8, device=mask.device)
    check(lib().m3d_binary_closing6_batch(_ptr(mask), _ptr(offsets), _ptr(dims.contiguous()), R, C.c_int64(total), _ptr(out),
                                          _ptr(ws), C.c_size_t(total + 512), _stream()), "binary_closing6_batch")
    return out


def paint_instances_into(vol, mask, offsets, boxes, ids):
    """Accumulating form: vol is an int32 [D,H,W] volume pre-filled with -1 (0xFFFFFFFF); several calls (one per tile)
    may paint into it; finish with `torch.where(vol == -1, 0, vol)`."""
    _need_gpu(vol, mask, offsets, boxes, ids)
    assert vol.dtype == torch.int32 and vol.is_contiguous() and boxes.dtype == torch.int32 and ids.dtype == torch.int32
    D, H, W = vol.shape
    check(lib().m3d_paint_instances(_ptr(mask), _ptr(offsets), _ptr(boxes.contiguous()), _ptr(ids.contiguous()), boxes.shape[0],
                                    D, H, W, _ptr(vol), _stream()), "paint_instances")
    return vol


def paint_finish(vol, max_id, present=None):
    """In place: sentinel -> 0; returns bool [max_id + 1]: id occurs in the volume (index 0 unused).  No host synchronisation.
    present: a zeroed uint8 [max_id + 1] buffer (paint_begin's), else one is made here."""
    _need_gpu(vol)
    assert vol.dtype == torch.int32 and vol.is_contiguous()
    if present is None:
        present = torch.zeros((int(max_id) + 1,), dtype=torch.uint8, device=vol.device)
    assert present.numel() == int(max_id) + 1 and present.dtype == torch.uint8
    check(lib().m3d_paint_finish(_ptr(vol), C.c_int64(vol.numel()), int(max_id), _ptr(present), _stream()), "paint_finish")
    return present.view(torch.bool)


def crop_offsets(boxes_host):
    """int64 [R+1]: start of each box's crop in the concatenated crop buffers (boxes inclusive (x1,y1,z1,x2,y2,z2))."""
    b = np.asarray(boxes_host).astype(np.int64)
    sizes = (b[:, 3] - b[:, 0] + 1) * (b[:, 4] - b[:, 1] + 1) * (b[:, 5] - b[:, 2] + 1)
    return np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)


def paint_begin(shape, num_present, st_otsu, st_cc, map_stats, idx, first_id, device):
    """One launch: label volume int32 [D,H,W] at the 0xFFFFFFFF sentinel, present uint8 [num_present] at 0, ids int32 [R] (idx + first_id,
    -1 where a stage failed or the detection's map is all zero).  Returns (volume, present, ids)."""
    _need_gpu(st_otsu, st_cc, idx)
    R = int(idx.numel())
    assert idx.dtype == torch.int64 and st_otsu.dtype == torch.int32 and st_cc.dtype == torch.int32 and st_otsu.numel() == R == st_cc.numel()
    vol = torch.empty(tuple(shape), dtype=torch.int32, device=device)
    present = torch.empty((int(num_present),), dtype=torch.uint8, device=device)
    ids = torch.empty((R,), dtype=torch.int32, device=device)
    if map_stats is not None:
        assert map_stats.dtype == torch.int32 and map_stats.is_contiguous()
    check(lib().m3d_paint_begin(_ptr(vol), C.c_int64(vol.numel()), _ptr(present), int(num_present), _ptr(st_otsu), _ptr(st_cc), _ptr(map_stats),
                                _ptr(idx), R, int(first_id), _ptr(ids), _stream()), "paint_begin")
    return vol, present, ids


def paint_instances(mask, offsets, boxes, ids, shape):
    """Returns the int32 label volume [D,H,W]: id of the first (lowest-id) instance covering each voxel, 0 elsewhere.
    ids < 0 (0xFFFFFFFF as unsigned) never win, i.e. mark a skipped detection."""
    vol = torch.full(tuple(shape), -1, dtype=torch.int32, device=mask.device)      # 0xFFFFFFFF sentinel
    paint_instances_into(vol, mask, offsets, boxes, ids)
    return torch.where(vol == -1, torch.zeros_like(vol), vol)


# ------------------------------------------------------------------ evaluation of label volumes (csrc/eval3d.hip)
LABEL_LIMIT = 1 << 24            # labels must lie in [0, 2^24): (a, b) pairs are 48-bit hash keys
_OVERLAP_DEFAULT_SLOTS = 1 << 16


def _label_volume(x):
    """A label volume as a contiguous CUDA tensor and its label width in bytes: uint16 (what the TIFFs hold) or int32 (what
    m3d_paint_* produce).  NumPy arrays are uploaded; bool / uint8 widen to uint16, wider integers are range-checked into int32."""
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x)
        if x.dtype in (np.bool_, np.uint8):
            x = x.astype(np.uint16)
        elif x.dtype not in (np.uint16, np.int32):
            if x.dtype.kind not in "iu":
                raise ValueError("label volumes hold integers, got %s" % x.dtype)
            if x.size and (int(x.min()) < 0 or int(x.max()) >= LABEL_LIMIT):
                raise M3DError("labels must lie in [0, 2^24)")
            x = x.astype(np.int32)
        x = torch.from_numpy(x).cuda()
    _need_gpu(x)
    x = x.contiguous()
    if x.dtype in (torch.bool, torch.uint8):
        x = x.to(torch.int16)
    elif x.dtype not in (torch.uint16, torch.int16, torch.int32):
        if x.numel() and (int(x.min()) < 0 or int(x.max()) >= LABEL_LIMIT):
            raise M3DError("labels must lie in [0, 2^24)")
        x = x.to(torch.int32)
    return x, x.element_size()


def _widen(x):
    """2-byte labels (read as uint16) -> int32"""
    return x if x.element_size() == 4 else (x.view(torch.int16).to(torch.int32) & 0xFFFF)


def _label_max(x, nbytes):
    """The default declared maximum: the dtype's for uint16 (no extra pass; 64 K counts), the volume's own for int32."""
    if nbytes == 2:
        return 65535
    m = int(x.max()) if x.numel() else 0
    if m >= LABEL_LIMIT:
        raise M3DError("label %d >= 2^24" % m)
    return max(m, 0)


class Overlap(tuple):
    """(count_a int64 [max_a + 1], count_b int64 [max_b + 1], pairs int32 [P, 2] sorted by (a, b), counts int64 [P]) on the device."""
    __slots__ = ()

    def __new__(cls, count_a, count_b, pairs, counts):
        return tuple.__new__(cls, (count_a, count_b, pairs, counts))

    count_a = property(lambda s: s[0])
    count_b = property(lambda s: s[1])
    pairs = property(lambda s: s[2])
    counts = property(lambda s: s[3])


def label_overlap(a, b, max_a=None, max_b=None, capacity=None):
    """Contingency table of two label volumes of the same shape (m3d_label_overlap): voxel counts per label on each side and every
    (a, b) pair with a > 0 and b > 0 that occurs, sorted by (a, b).  max_a / max_b: the declared label maxima (None: 65535 for uint16
    labels, the volume's maximum for int32); a label above them raises M3DError.  capacity: hash-table slots (a power of two; default
    64 K): when the pairs do not fit, the call re-launches once with the proven bound min(V, (max_a + 1)(max_b + 1)).
    Synchronises (the number of pairs is data dependent).  Returns Overlap."""
    a, na = _label_volume(a)
    b, nb = _label_volume(b)
    if a.shape != b.shape:
        raise ValueError("label volumes differ in shape: %s vs %s" % (tuple(a.shape), tuple(b.shape)))
    if na != nb:
        a, b, na, nb = _widen(a), _widen(b), 4, 4
    max_a = _label_max(a, na) if max_a is None else int(max_a)
    max_b = _label_max(b, nb) if max_b is None else int(max_b)
    if not (0 <= max_a < LABEL_LIMIT and 0 <= max_b < LABEL_LIMIT):
        raise M3DError("declared label maxima must lie in [0, 2^24)")
    V = a.numel()
    bound = max(1, min(V, (max_a + 1) * (max_b + 1)))
    full = 1 << (2 * bound - 1).bit_length()
    cap = min(full, _OVERLAP_DEFAULT_SLOTS) if capacity is None else int(capacity)
    if cap <= 0 or cap & (cap - 1):
        raise ValueError("capacity must be a power of two")
    dev = a.device
    count_a = torch.empty((max_a + 1,), dtype=torch.int64, device=dev)
    count_b = torch.empty((max_b + 1,), dtype=torch.int64, device=dev)
    status = torch.empty((2,), dtype=torch.int64, device=dev)
    for attempt in range(2):
        wsb = int(lib().m3d_label_overlap_workspace_bytes(max_a, C.c_int64(cap)))
        ws = torch.empty((max(wsb, 256),), dtype=torch.uint8, device=dev)
        pairs = torch.empty((cap, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((cap,), dtype=torch.int64, device=dev)
        check(lib().m3d_label_overlap(_ptr(a), _ptr(b), na, C.c_int64(V), max_a, max_b, C.c_int64(cap), _ptr(count_a), _ptr(count_b),
                                      _ptr(pairs), _ptr(counts), _ptr(status), _ptr(ws), C.c_size_t(wsb), _stream()), "label_overlap")
        flags, npairs = (int(v) for v in status.cpu())
        if flags & 1:
            raise M3DError("label_overlap: a label lies above the declared maximum (%d, %d) or outside [0, 2^24)" % (max_a, max_b))
        if not flags & 2:
            return Overlap(count_a, count_b, pairs[:npairs], counts[:npairs])
        if attempt == 0:
            cap = full          # the proven bound, once
    raise M3DError("label_overlap: the hash table of %d slots was full at the proven bound" % cap)


class IouBest(tuple):
    """(max_iou fp32 [R], argmax int32 [R], iou fp32 [R, G] or None) on the device, gt_ids int64 ndarray [G] (column -> GT id)."""
    __slots__ = ()

    def __new__(cls, max_iou, argmax, iou, gt_ids):
        return tuple.__new__(cls, (max_iou, argmax, iou, gt_ids))

    max_iou = property(lambda s: s[0])
    argmax = property(lambda s: s[1])
    iou = property(lambda s: s[2])
    gt_ids = property(lambda s: s[3])


def label_iou_best(overlap, row_ids, gt_ids=None, dense=False):
    """Per row (a pred id; rows in the caller's order, ids may be absent from the volume: an empty mask) the IoU with every GT column,
    computed as mask_iou_fast does (fp64 counts, one fp32 rounding; m3d_label_iou_best): its largest fp32 value and the lowest column
    holding it (0 for a row without overlap), and with dense=True the [R, G] matrix.  gt_ids: the column ids (default: the non-zero
    labels present on the GT side, ascending - eval_instance_segmentation_soma.py:181-182)."""
    count_a, count_b, pairs, counts = overlap
    _need_gpu(count_a, count_b, pairs, counts)
    dev = count_a.device
    max_a, max_b = count_a.numel() - 1, count_b.numel() - 1
    if gt_ids is None:
        cb = count_b.cpu().numpy()
        gt_ids = np.nonzero(cb[1:] > 0)[0].astype(np.int64) + 1
    gt_ids = np.asarray(gt_ids, dtype=np.int64).reshape(-1)
    if gt_ids.size and (gt_ids.min() < 1 or gt_ids.max() > max_b or np.unique(gt_ids).size != gt_ids.size):
        raise ValueError("gt_ids must be distinct ids in [1, %d]" % max_b)
    col = np.full((max_b + 1,), -1, dtype=np.int32)
    col[gt_ids] = np.arange(gt_ids.size, dtype=np.int32)
    rows = np.asarray(row_ids.cpu() if torch.is_tensor(row_ids) else row_ids).astype(np.int64).reshape(-1)
    if rows.size and (rows.min() < 1 or rows.max() >= 2 ** 31):
        raise ValueError("row ids must be positive pred ids")
    R, G = rows.size, gt_ids.size
    col_d, rows_d = upload_packed([col, rows.astype(np.int32)], dev)
    max_iou = torch.empty((R,), dtype=torch.float32, device=dev)
    argmax = torch.empty((R,), dtype=torch.int32, device=dev)
    iou = torch.empty((R, G), dtype=torch.float32, device=dev) if dense else None
    check(lib().m3d_label_iou_best(_ptr(pairs), _ptr(counts), C.c_int64(pairs.shape[0]), _ptr(count_a), max_a, _ptr(count_b), max_b,
                                   _ptr(col_d), G, _ptr(rows_d), R, _ptr(max_iou), _ptr(argmax), _ptr(iou), _stream()), "label_iou_best")
    return IouBest(max_iou, argmax, iou, gt_ids)


def box_union_overlap_counts(a, b, ranges):
    """(Σ(a > 0), Σ(b > 0), Σ(a > 0 & b > 0 & inside at least one box)) of two [D, H, W] volumes (m3d_box_union_overlap_counts);
    ranges int [K, 6] = half-open (z0, z1, y0, y1, x0, x1), already normalised by the caller.  Synchronises; returns int64 ndarray [3]."""
    a, na = _label_volume(a)
    b, nb = _label_volume(b)
    if a.dim() != 3 or a.shape != b.shape:
        raise ValueError("box_union_overlap_counts needs two [D, H, W] volumes of one shape")
    if na != nb:
        a, b, na = _widen(a), _widen(b), 4
    D, H, W = (int(v) for v in a.shape)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.int64).reshape(-1, 6))
    K = r.shape[0]
    dev = a.device
    r_d = upload_packed([r.astype(np.int32)], dev)[0] if K else None
    out = torch.empty((3,), dtype=torch.int64, device=dev)
    wsb = int(lib().m3d_box_union_overlap_workspace_bytes(C.c_int64(D * H * W)))
    ws = torch.empty((max(wsb, 256),), dtype=torch.uint8, device=dev)
    check(lib().m3d_box_union_overlap_counts(_ptr(a), _ptr(b), na, D, H, W, _ptr(r_d), K, _ptr(out), _ptr(ws), C.c_size_t(wsb), _stream()),
          "box_union_overlap_counts")
    return out.cpu().numpy()


# ------------------------------------------------------------------ whole-volume labelling, sphere painting (csrc/label3d.hip)
_COMPONENT_DTYPES = {np.dtype(np.uint8): 1, np.dtype(np.uint16): 2, np.dtype(np.int32): 4}


def _component_volume(x):
    """A [D, H, W] volume of uint8 / uint16 / int32 (bool counts as uint8) as a contiguous CUDA tensor and its element size.  Other
    dtypes and other ranks raise ValueError: nothing is converted silently, since equal VALUES are what connects."""
    if isinstance(x, np.ndarray):
        if x.dtype == np.bool_:
            x = x.view(np.uint8)
        if x.dtype not in _COMPONENT_DTYPES:
            raise ValueError("label_components takes bool, uint8, uint16 or int32 volumes, got %s" % x.dtype)
        if x.ndim != 3:
            raise ValueError("label_components takes a [D, H, W] volume, got %d dimensions" % x.ndim)
        return torch.from_numpy(np.ascontiguousarray(x)).cuda(), _COMPONENT_DTYPES[x.dtype]
    if not torch.is_tensor(x):
        raise ValueError("label_components takes a NumPy array or a CUDA tensor")
    if x.dtype == torch.bool:
        x = x.to(torch.uint8)
    if x.dtype not in (torch.uint8, torch.uint16, torch.int16, torch.int32):
        raise ValueError("label_components takes bool, uint8, uint16 or int32 volumes, got %s" % x.dtype)
    if x.dim() != 3:
        raise ValueError("label_components takes a [D, H, W] volume, got %d dimensions" % x.dim())
    _need_gpu(x)
    return x.contiguous(), x.element_size()


def label_counts(labels, num_labels):
    """Voxels per label of an int32 CUDA label volume: int64 [num_labels + 1] on the device (m3d_label_counts).  No synchronisation."""
    _need_gpu(labels)
    if labels.dtype != torch.int32:
        raise ValueError("label_counts takes int32 labels")
    labels = labels.contiguous()
    counts = torch.empty((int(num_labels) + 1,), dtype=torch.int64, device=labels.device)
    check(lib().m3d_label_counts(_ptr(labels), C.c_int64(labels.numel()), int(num_labels), _ptr(counts), _stream()), "label_counts")
    return counts


def label_components(volume, connectivity=26, return_counts=False):
    """Connected components of a whole [D, H, W] volume with skimage.measure.label's default semantics (m3d_label_components): a
    component is a maximal `connectivity`-connected (6, 18 or 26) set of voxels sharing one non-zero value; 0 is background.  Labels
    are 1..K in the raster order of each component's first voxel.  volume: NumPy or CUDA, bool / uint8 / uint16 / int32.
    Returns (labels int32 CUDA [D, H, W], K) and, with return_counts, counts int64 CUDA [K + 1].  Synchronises once, for K."""
    x, nbytes = _component_volume(volume)
    D, H, W = (int(v) for v in x.shape)
    return _label_components_raw(x, nbytes, D, H, W, connectivity, return_counts)


def _label_components_raw(x, nbytes, D, H, W, connectivity, return_counts=False):
    """The call itself; the argument checks are the library's (tests reach them with shape arguments alone)."""
    V = D * H * W
    dev = x.device
    big = V >= 2 ** 31 or V <= 0                       # refused by the library before any launch: nothing of that size is allocated
    labels = torch.empty((1,) if big else (D, H, W), dtype=torch.int32, device=dev)
    num = torch.empty((1,), dtype=torch.int32, device=dev)
    wsb = 256 if big else int(lib().m3d_label_components_workspace_bytes(C.c_int64(V)))
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib().m3d_label_components(_ptr(x), int(nbytes), D, H, W, int(connectivity), _ptr(labels), _ptr(num), _ptr(ws), C.c_size_t(wsb),
                                     _stream()), "label_components")
    K = int(num.item())
    if return_counts:
        return labels, K, label_counts(labels, K)
    return labels, K


def paint_spheres(spheres, shape):
    """NeuroGPS soma lists as a label volume (m3d_paint_spheres; eval_instance_segmentation_soma_ngps.py:160-183): spheres int [N, 4] =
    (x, y, z, r), sphere i paints id i + 1 where r >= 6, never at index 0 of an axis, the highest index winning where spheres overlap.
    Returns uint16 CUDA [S, H, W].  More than 65 535 spheres raise M3DError."""
    sp = np.ascontiguousarray(np.asarray(spheres.cpu() if torch.is_tensor(spheres) else spheres, dtype=np.int64).reshape(-1, 4))
    if sp.size and (sp.min() < -2 ** 31 or sp.max() >= 2 ** 31):
        raise ValueError("sphere fields must fit int32")
    S, H, W = (int(v) for v in shape)
    N = sp.shape[0]
    dev = torch.device("cuda")
    sp_d = upload_packed([sp.astype(np.int32)], dev)[0] if N else None
    V = S * H * W
    out = torch.empty((S, H, W) if 0 < V < 2 ** 31 else (1,), dtype=torch.uint16, device=dev)
    wsb = int(lib().m3d_paint_spheres_workspace_bytes(C.c_int64(V))) if 0 < V < 2 ** 31 else 256
    ws = torch.empty((wsb,), dtype=torch.uint8, device=dev)
    check(lib().m3d_paint_spheres(_ptr(sp_d), N, S, H, W, _ptr(out), _ptr(ws), C.c_size_t(wsb), _stream()), "paint_spheres")
    return out


# ------------------------------------------------------------------ RPN training step (csrc/rpn_train.hip)
def rpn_target_sets(cell_anchors, field_size, stride, gt_boxes, dc_boxes, im_size, straddle_thresh, positive_overlap, negative_overlap,
                batch_per_im, num_fg, seed):
    """m3d_rpn_targets for one image: gt_boxes / dc_boxes CUDA fp32 [K,6] (dc_boxes may be None), im_size = (slices, height, width),
    cell_anchors host fp64 [A,6].  -> (fg_index int64 [num_fg], bg_index int64 [batch_per_im], target_index int64 [num_fg],
    targets fp32 [num_fg,6], counts int64 [8]), all on the device, no synchronisation."""
    _need_gpu(gt_boxes, dc_boxes)
    gt = _f32c(gt_boxes).reshape(-1, 6)
    dc = _f32c(dc_boxes).reshape(-1, 6) if dc_boxes is not None else None
    cell = np.ascontiguousarray(cell_anchors, np.float64).reshape(-1, 6)
    A, F, dev = cell.shape[0], int(field_size), gt.device
    fg = torch.empty((num_fg,), dtype=torch.int64, device=dev)
    bg = torch.empty((batch_per_im,), dtype=torch.int64, device=dev)
    tix = torch.empty((num_fg,), dtype=torch.int64, device=dev)
    tg = torch.empty((num_fg, 6), dtype=torch.float32, device=dev)
    counts = torch.empty((8,), dtype=torch.int64, device=dev)
    L = lib()
    nbytes = L.m3d_rpn_targets_workspace_bytes(A, F, gt.shape[0], int(batch_per_im), int(num_fg))
    ws = _workspace(max(int(nbytes), 1), dev, "rpn_targets")
    S, H, W = [float(v) for v in im_size]
    check(L.m3d_rpn_targets(cell.ctypes.data_as(C.POINTER(C.c_double)), A, F, int(stride), _ptr(gt if gt.shape[0] else None), gt.shape[0],
                            _ptr(dc if dc is not None and dc.shape[0] else None), 0 if dc is None else dc.shape[0], C.c_double(S),
                            C.c_double(H), C.c_double(W), C.c_double(float(straddle_thresh)), C.c_double(float(positive_overlap)),
                            C.c_double(float(negative_overlap)), int(batch_per_im), int(num_fg), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                            _ptr(fg), _ptr(bg), _ptr(tix), _ptr(tg), _ptr(counts), _ptr(ws), C.c_size_t(ws.numel()), _stream()),
          "rpn_targets")
    return fg, bg, tix, tg, counts


def rpn_target_blobs(fg_index, bg_index, target_index, targets, counts, num_cell_anchors, field_size):
    """The reference's four dense blobs (rpn.py:260-278): labels int32 [1,A,F,F,F], targets / inside / outside weights fp32 [1,6A,F,F,F]."""
    _need_gpu(fg_index, bg_index, target_index, targets, counts)
    A, F, dev = int(num_cell_anchors), int(field_size), bg_index.device
    lab = torch.empty((1, A, F, F, F), dtype=torch.int32, device=dev)
    tw, iw, ow = (torch.empty((1, 6 * A, F, F, F), dtype=torch.float32, device=dev) for _ in range(3))
    check(lib().m3d_rpn_targets_wide(_ptr(fg_index), _ptr(bg_index), _ptr(target_index), _ptr(targets), _ptr(counts), A, F,
                                     fg_index.shape[0], bg_index.shape[0], _ptr(lab), _ptr(tw), _ptr(iw), _ptr(ow), _stream()),
          "rpn_targets_wide")
    return lab, tw, iw, ow


def rpn_loss_grad(cls_logits, bbox_pred, field_size, fg_index, bg_index, target_index, targets, counts):
    """m3d_rpn_loss: cls_logits [B,A,s,h,w], bbox_pred [B,6A,s,h,w]; the per-image outputs of rpn_target_sets stacked along a leading B.
    -> (losses fp32 [2] = (loss_cls, loss_bbox), d loss_cls / d cls_logits, d loss_bbox / d bbox_pred)."""
    _need_gpu(cls_logits, bbox_pred, fg_index, bg_index, target_index, targets, counts)
    x, p = _f32c(cls_logits), _f32c(bbox_pred)
    B, A, s, h, w = x.shape
    if tuple(p.shape) != (B, 6 * A, s, h, w) or fg_index.shape[0] != B or bg_index.shape[0] != B or counts.shape != (B, 8):
        raise M3DError("rpn_loss_grad: bbox_pred must be [B,6A,s,h,w] and the targets stacked over the same B images")
    fg_index, bg_index, target_index, targets, counts = (t.contiguous() for t in (fg_index, bg_index, target_index, targets, counts))
    losses = torch.empty((2,), dtype=torch.float32, device=x.device)
    gx, gp = torch.empty_like(x), torch.empty_like(p)
    check(lib().m3d_rpn_loss(_ptr(x), _ptr(p), B, A, s, h, w, int(field_size), _ptr(fg_index), _ptr(bg_index), _ptr(target_index),
                             _ptr(targets), _ptr(counts), fg_index.shape[1], bg_index.shape[1], _ptr(losses), _ptr(gx), _ptr(gp), _stream()),
          "rpn_loss")
    return losses, gx, gp


# ------------------------------------------------------------------ box-head training step (csrc/box_head_train.hip)
def box_head_target_sets(rois, num, gt, gt_offsets, gt_classes, gt_crowd, batch_per_im, fg_per_im, fg_thresh, bg_thresh_hi, bg_thresh_lo,
                         bbox_reg_weights, num_classes, seeds, cls_agnostic_bbox_reg=False):
    """m3d_box_head_targets for the B images of a minibatch: rois fp32 [B,rows,7] and num int32 [B] as generate_proposals3d_batched
    returns them, gt CUDA fp32 [sum K,6] with host offsets [B+1], gt_classes int32 / gt_crowd uint8 [sum K] or None, seeds: B host
    integers.  -> (rows int64 [B,batch], labels int32 [B,batch], rois fp32 [B,batch,6], targets fp32 [B,batch,6], counts int64 [B,8]),
    all on the device, no synchronisation."""
    _need_gpu(rois, num, gt, gt_classes, gt_crowd)
    rois, gt = _f32c(rois), _f32c(gt).reshape(-1, 6)
    if rois.dim() != 3 or rois.shape[2] != 7 or num.dtype != torch.int32 or tuple(num.shape) != (rois.shape[0],):
        raise M3DError("box_head_target_sets: rois must be [B,rows,7] and num int32 [B]")
    B, R, dev = rois.shape[0], rois.shape[1], rois.device
    off = np.ascontiguousarray(gt_offsets, np.int32)
    sd = np.array([int(s) & (2 ** 64 - 1) for s in seeds], np.uint64)
    if off.shape != (B + 1,) or sd.shape != (B,) or int(off[-1]) != gt.shape[0]:
        raise M3DError("box_head_target_sets: %d images need %d box offsets ending at %d and %d seeds" % (B, B + 1, gt.shape[0], B))
    for name, t, dt in (("gt_classes", gt_classes, torch.int32), ("gt_crowd", gt_crowd, torch.uint8)):
        if t is not None and (t.dtype != dt or t.numel() != gt.shape[0] or not t.is_contiguous()):
            raise M3DError("box_head_target_sets: %s must be a contiguous %s tensor with one entry per box" % (name, dt))
    wt = np.ascontiguousarray(bbox_reg_weights, np.float64)
    if wt.shape != (6,):
        raise M3DError("box_head_target_sets: six bbox_reg_weights")
    num = num.contiguous()
    batch = int(batch_per_im)
    rows = torch.empty((B, batch), dtype=torch.int64, device=dev)
    labels = torch.empty((B, batch), dtype=torch.int32, device=dev)
    out_rois = torch.empty((B, batch, 6), dtype=torch.float32, device=dev)
    targets = torch.empty((B, batch, 6), dtype=torch.float32, device=dev)
    counts = torch.empty((B, 8), dtype=torch.int64, device=dev)
    L = lib()
    max_gt = int(np.diff(off).max()) if B else 0
    nbytes = L.m3d_box_head_targets_workspace_bytes(B, max_gt, R)
    ws = _workspace(max(int(nbytes), 1), dev, "box_head_targets")
    check(L.m3d_box_head_targets(_ptr(gt if gt.shape[0] else None), _ptr(gt_classes), _ptr(gt_crowd), off.ctypes.data_as(C.c_void_p), B,
                                 _ptr(rois if R else None), _ptr(num), R, batch, int(fg_per_im), C.c_double(float(fg_thresh)),
                                 C.c_double(float(bg_thresh_hi)), C.c_double(float(bg_thresh_lo)), wt.ctypes.data_as(C.c_void_p),
                                 int(num_classes), int(bool(cls_agnostic_bbox_reg)), sd.ctypes.data_as(C.c_void_p), _ptr(rows),
                                 _ptr(labels), _ptr(out_rois), _ptr(targets), _ptr(counts), _ptr(ws), C.c_size_t(ws.numel()), _stream()),
          "box_head_targets")
    return rows, labels, out_rois, targets, counts


def box_head_target_blobs(labels, targets, num_classes):
    """_expand_bbox_targets on the device: labels int32 [...], targets fp32 [...,6] -> bbox_targets, bbox_inside_weights,
    bbox_outside_weights fp32 [N, 6 num_classes] with N = labels.numel()."""
    _need_gpu(labels, targets)
    labels, targets = labels.contiguous(), _f32c(targets)
    N = labels.numel()
    if labels.dtype != torch.int32 or targets.numel() != 6 * N:
        raise M3DError("box_head_target_blobs: labels int32 [N] and targets [N,6]")
    bt, iw, ow = (torch.empty((N, 6 * int(num_classes)), dtype=torch.float32, device=labels.device) for _ in range(3))
    check(lib().m3d_box_head_target_blobs(_ptr(labels), _ptr(targets), C.c_int64(N), int(num_classes), _ptr(bt), _ptr(iw), _ptr(ow),
                                          _stream()), "box_head_target_blobs")
    return bt, iw, ow


def box_head_loss_grad(cls_score, bbox_pred, labels, targets, counts):
    """m3d_box_head_loss: cls_score [B batch, C], bbox_pred [B batch, 6 C]; labels [B,batch], targets [B,batch,6], counts [B,8] of
    box_head_target_sets.  -> (losses fp32 [3] = (loss_cls, loss_bbox, accuracy_cls), d loss_cls / d cls_score, d loss_bbox / d bbox_pred)."""
    _need_gpu(cls_score, bbox_pred, labels, targets, counts)
    x, p = _f32c(cls_score), _f32c(bbox_pred)
    if labels.dim() != 2 or x.dim() != 2 or p.dim() != 2:
        raise M3DError("box_head_loss_grad: cls_score [B batch, C], bbox_pred [B batch, 6 C], labels [B, batch]")
    B, batch = labels.shape
    N, Cn = x.shape
    if N != B * batch or tuple(p.shape) != (N, 6 * Cn) or tuple(targets.shape) != (B, batch, 6) or tuple(counts.shape) != (B, 8):
        raise M3DError("box_head_loss_grad: %s scores and %s predictions for %d x %d sampled rows" % (tuple(x.shape), tuple(p.shape), B, batch))
    if labels.dtype != torch.int32 or counts.dtype != torch.int64 or targets.dtype != torch.float32:
        raise M3DError("box_head_loss_grad: labels int32, targets fp32, counts int64")
    labels, targets, counts = labels.contiguous(), targets.contiguous(), counts.contiguous()
    losses = torch.empty((3,), dtype=torch.float32, device=x.device)
    gx, gp = torch.empty_like(x), torch.empty_like(p)
    check(lib().m3d_box_head_loss(_ptr(x), _ptr(p), _ptr(labels), _ptr(targets), _ptr(counts), B, batch, Cn, _ptr(losses), _ptr(gx), _ptr(gp),
                                  _stream()), "box_head_loss")
    return losses, gx, gp


# ------------------------------------------------------------------ mask-branch training step (csrc/mask_train.hip)
MASK_SPOT, MASK_LABELS = 0, 1


def mask_target_sets(labels, rois, counts, gt_offsets, fg_per_im, resolution, num_classes, cls_specific, spots=None, in_size=None,
                     gt=None, markers=None, volumes=None, gt_classes=None, gt_crowd=None):
    """m3d_mask_targets for the B images of a minibatch: labels int32 [B,batch], rois fp32 [B,batch,6], counts int64 [B,8] of
    box_head_target_sets; host offsets [B+1] into the concatenated objects.  Spot mode: spots CUDA fp32 [sum K,4] (x, y, z, r) and in_size
    (slices, height, width).  Mask mode: gt CUDA fp32 [sum K,6], markers int32 [sum K], volumes: per image a CUDA uint16 / int32 label
    volume [D,H,W].  -> (masks int32 [B,fg_per_im,Cm M^3], rois fp32 [B,fg_per_im,6], assign int32 [B,fg_per_im], counts int64 [B,4]),
    all on the device, no synchronisation."""
    _need_gpu(labels, rois, counts, spots, gt, markers, gt_classes, gt_crowd)
    if (spots is None) == (gt is None):
        raise M3DError("mask_target_sets: either spots (spot mode) or gt boxes, markers and label volumes (mask mode)")
    if labels.dim() != 2 or labels.dtype != torch.int32 or counts.dtype != torch.int64 or tuple(counts.shape) != (labels.shape[0], 8) or \
            tuple(rois.shape) != tuple(labels.shape) + (6,) or rois.dtype != torch.float32:
        raise M3DError("mask_target_sets: labels int32 [B,batch], rois fp32 [B,batch,6], counts int64 [B,8]")
    labels, rois, counts = labels.contiguous(), rois.contiguous(), counts.contiguous()
    B, batch, dev = labels.shape[0], labels.shape[1], labels.device
    off = np.ascontiguousarray(gt_offsets, np.int32)
    if off.shape != (B + 1,):
        raise M3DError("mask_target_sets: %d images need %d object offsets" % (B, B + 1))
    total = int(off[-1])
    for name, t, dt, width in (("spots", spots, torch.float32, 4), ("gt", gt, torch.float32, 6), ("markers", markers, torch.int32, 1),
                               ("gt_classes", gt_classes, torch.int32, 1), ("gt_crowd", gt_crowd, torch.uint8, 1)):
        if t is not None and (t.dtype != dt or t.numel() != total * width or not t.is_contiguous()):
            raise M3DError("mask_target_sets: %s must be a contiguous %s tensor with %d value(s) per object, %d objects" % (name, dt, width, total))
    images, size = None, None
    if spots is not None:
        size = (C.c_int32 * 3)(*[int(v) for v in in_size])
        mode = MASK_SPOT
    else:
        if markers is None or volumes is None or len(volumes) != B:
            raise M3DError("mask_target_sets: mask mode needs markers and one label volume per image")
        images = (MaskImage * B)()
        for b, v in enumerate(volumes):
            if v is None:
                continue
            _need_gpu(v)
            if v.dim() != 3 or v.dtype not in (torch.uint16, torch.int32) or not v.is_contiguous():
                raise M3DError("mask_target_sets: a label volume is a contiguous uint16 or int32 [D,H,W] tensor")
            images[b].labels, images[b].dtype = v.data_ptr(), 0 if v.dtype == torch.uint16 else 1
            images[b].depth, images[b].height, images[b].width = (int(x) for x in v.shape)
        mode = MASK_LABELS
    M, F = int(resolution), int(fg_per_im)
    Cm = int(num_classes) if cls_specific else 1
    shape_ok = 2 <= M <= 32 and 1 <= F <= 4096 and 1 <= Cm <= 64
    masks = torch.empty((B, F, Cm * M ** 3) if shape_ok else (1,), dtype=torch.int32, device=dev)
    out_rois = torch.empty((B, F, 6) if shape_ok else (1,), dtype=torch.float32, device=dev)
    assign = torch.empty((B, F) if shape_ok else (1,), dtype=torch.int32, device=dev)
    mcounts = torch.empty((B, 4), dtype=torch.int64, device=dev)
    check(lib().m3d_mask_targets(_ptr(labels), _ptr(rois), _ptr(counts), B, batch, F, M, int(num_classes), int(bool(cls_specific)), mode,
                                 off.ctypes.data_as(C.c_void_p), _ptr(gt_classes), _ptr(gt_crowd), _ptr(spots), size, _ptr(gt),
                                 _ptr(markers), images, _ptr(masks), _ptr(out_rois), _ptr(assign), _ptr(mcounts), _stream()),
          "mask_targets")
    return masks, out_rois, assign, mcounts


def mask_loss_grad(mask_pred, masks, weight_loss_mask=1.0):
    """m3d_mask_loss: mask_pred fp32 [N,Cm,M,M,M], masks int32 with N Cm M^3 elements (-1 = ignore).
    -> (loss fp32 [1], number of labelled elements int64 [1], d loss / d mask_pred)."""
    _need_gpu(mask_pred, masks)
    x = _f32c(mask_pred)
    if x.dim() != 5 or x.shape[2] != x.shape[3] or x.shape[3] != x.shape[4] or masks.dtype != torch.int32 or masks.numel() != x.numel():
        raise M3DError("mask_loss_grad: mask_pred [N,Cm,M,M,M] and int32 masks of the same element count, got %s and %s %s"
                       % (tuple(x.shape), masks.dtype, tuple(masks.shape)))
    masks = masks.contiguous()
    N, Cm, M = int(x.shape[0]), int(x.shape[1]), int(x.shape[2])
    L = lib()
    nbytes = int(L.m3d_mask_loss_workspace_bytes(C.c_int64(N), Cm, M))
    ws = _workspace(max(nbytes, 1), x.device, "mask_loss")
    loss = torch.empty((1,), dtype=torch.float32, device=x.device)
    num = torch.empty((1,), dtype=torch.int64, device=x.device)
    gx = torch.empty_like(x)
    check(L.m3d_mask_loss(_ptr(x), _ptr(masks), C.c_int64(N), Cm, M, C.c_double(float(weight_loss_mask)), _ptr(loss), _ptr(num), _ptr(gx),
                          _ptr(ws), C.c_size_t(ws.numel()), _stream()), "mask_loss")
    return loss, num, gx


# ------------------------------------------------------------------ BatchNorm3d on batch statistics (csrc/bn_train.hip)
def _bn_input(x, what):
    _need_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 5 or not x.is_contiguous():
        raise M3DError("%s: x must be a contiguous fp32 [N,C,D,H,W] tensor" % what)
    return tuple(int(v) for v in x.shape)


def _bn_vec(t, C, what, name):
    _need_gpu(t)
    if t.dtype != torch.float32 or tuple(t.shape) != (C,):
        raise M3DError("%s: %s must be fp32 [%d]" % (what, name, C))
    return t.contiguous()


def _bn_ws(call, device, tag):
    """two-step workspace protocol of csrc/bn_train.hip: ask with d_ws = NULL, then launch"""
    need = C.c_size_t(0)
    check(call(C.c_void_p(0), C.byref(need)), tag)
    ws = _workspace(max(int(need.value), 8), device, tag)
    cap = C.c_size_t(ws.numel())
    check(call(_ptr(ws), C.byref(cap)), tag)


def bn_stats(x, eps=1e-5, running_mean=None, running_var=None, momentum=0.0):
    """m3d_bn_stats: per-channel (mean, biased var, invstd = 1 / sqrt(var + eps)) of x fp32 [N,C,D,H,W], fp32 [C] each; fp64 sums in a
    fixed order, bit-identical run to run.  running_mean / running_var (contiguous fp32 [C]), if given, are updated in place by
    `momentum` as torch.nn.BatchNorm3d updates them.  A non-contiguous x is copied."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise M3DError("bn_stats: x must be a CUDA (ROCm) tensor; there is no CPU path")
    x = x.contiguous()
    N, Cn, D, H, W = _bn_input(x, "bn_stats")
    for t in (running_mean, running_var):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != (Cn,) or not t.is_contiguous()):
            raise M3DError("bn_stats: running statistics must be contiguous CUDA fp32 [%d]" % Cn)
    mean, var, invstd = (torch.empty((Cn,), dtype=torch.float32, device=x.device) for _ in range(3))
    L, st = lib(), _stream()
    _bn_ws(lambda ws, nb: L.m3d_bn_stats(_ptr(x), N, Cn, D, H, W, C.c_double(float(eps)), _ptr(running_mean), _ptr(running_var),
                                            C.c_double(float(momentum)), _ptr(mean), _ptr(var), _ptr(invstd), ws, nb, st),
           x.device, "bn_stats")
    return mean, var, invstd


def bn_invstd(var, eps=1e-5):
    """fp32(1 / sqrt(fp64(var) + eps)) per channel: the invstd of given (running) variances, as bn_stats computes its own."""
    var = _bn_vec(var, var.numel(), "bn_invstd", "var")
    out = torch.empty_like(var)
    check(lib().m3d_bn_invstd(_ptr(var), var.numel(), C.c_double(float(eps)), _ptr(out), _stream()), "bn_invstd")
    return out


def bn_apply(x, mean, invstd, weight, bias, relu=True, pool=False):
    """m3d_bn_apply: y = (x - mean) * (weight * invstd) + bias [-> ReLU] [-> MaxPool3d(2,2)] in one pass.  -> y, or with pool
    (y_pooled, uint8 argmax); the un-pooled tensor is never stored."""
    N, Cn, D, H, W = _bn_input(x, "bn_apply")
    mean, invstd, weight, bias = (_bn_vec(t, Cn, "bn_apply", n) for t, n in ((mean, "mean"), (invstd, "invstd"), (weight, "weight"), (bias, "bias")))
    if pool:
        y = torch.empty((N, Cn, D // 2, H // 2, W // 2), dtype=torch.float32, device=x.device)
        am = torch.empty(y.shape, dtype=torch.uint8, device=x.device)
    else:
        y, am = torch.empty_like(x), None
    check(lib().m3d_bn_apply(_ptr(x), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(bias), N, Cn, D, H, W, int(bool(relu)), int(bool(pool)),
                             _ptr(y), _ptr(am), _stream()), "bn_apply")
    return (y, am) if pool else y


def bn_backward(x, mean, invstd, weight, bias, grad_out, argmax=None, relu=True, pool=False, training=True):
    """m3d_bn_backward: (grad_x, grad_weight, grad_bias) of bn_apply for grad_out of bn_apply's output shape (with pool: the pooled
    shape, and `argmax` as bn_apply returned it)."""
    N, Cn, D, H, W = _bn_input(x, "bn_backward")
    mean, invstd, weight, bias = (_bn_vec(t, Cn, "bn_backward", n) for t, n in ((mean, "mean"), (invstd, "invstd"), (weight, "weight"), (bias, "bias")))
    _need_gpu(grad_out, argmax)
    oshape = (N, Cn, D // 2, H // 2, W // 2) if pool else (N, Cn, D, H, W)
    if grad_out.dtype != torch.float32 or tuple(grad_out.shape) != oshape or not grad_out.is_contiguous():
        raise M3DError("bn_backward: grad_out must be a contiguous fp32 tensor of shape %s" % (oshape,))
    if pool and (argmax is None or argmax.dtype != torch.uint8 or tuple(argmax.shape) != oshape or not argmax.is_contiguous()):
        raise M3DError("bn_backward: pool needs the contiguous uint8 argmax of bn_apply")
    gx = torch.empty_like(x)
    gw, gb = (torch.empty((Cn,), dtype=torch.float32, device=x.device) for _ in range(2))
    L, st = lib(), _stream()
    _bn_ws(lambda ws, nb: L.m3d_bn_backward(_ptr(x), _ptr(mean), _ptr(invstd), _ptr(weight), _ptr(bias), _ptr(grad_out),
                                            _ptr(argmax if pool else None), N, Cn, D, H, W, int(bool(relu)), int(bool(pool)),
                                            int(bool(training)), _ptr(gx), _ptr(gw), _ptr(gb), ws, nb, st), x.device, "bn_backward")
    return gx, gw, gb


# ------------------------------------------------------------------ the solver's parameter update (csrc/sgd.hip)
def sgd_chunk():
    """elements of one tensor that one workgroup of m3d_sgd_step updates (the partition of its statistics)"""
    return int(lib().m3d_sgd_chunk())


def sgd_step(params, grads, bufs, lrs, wds, momentum, mscale=1.0, stats=None):
    """m3d_sgd_step: one fused SGD update of a whole parameter list, in place and on the current stream.

    params, grads: lists of contiguous CUDA fp32 tensors of equal sizes; bufs: the momentum buffers (same sizes), or None with momentum
    == 0; lrs, wds: one float per tensor.  Per element c = mscale m, d = g + wd p (g where wd == 0), m' = momentum c + d, p' = p - lr m',
    every fp32 operation rounded once.  stats: None, or a CUDA fp64 [2] tensor that receives (sum of g^2, number of non-finite gradient
    elements).  The update goes through raw pointers and does not bump the tensors' `_version`: the caller drops what it cached on them
    (m3d.compat.invalidate_packs(); m3d.Solver.step does)."""
    n = len(params)
    if bufs is None:
        bufs = [None] * n
    if not (len(grads) == len(bufs) == len(lrs) == len(wds) == n):
        raise M3DError("sgd_step: params, grads, bufs, lrs and wds must have one entry per tensor")
    arr = (SgdTensor * max(n, 1))()
    for i in range(n):
        p, g, m = params[i], grads[i], bufs[i]
        for t, name in ((p, "params"), (g, "grads"), (m, "bufs")):
            if t is None and name == "bufs":
                continue
            if not torch.is_tensor(t) or not t.is_cuda:
                raise M3DError("sgd_step: %s[%d] must be a CUDA (ROCm) tensor; there is no CPU path" % (name, i))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise M3DError("sgd_step: %s[%d] must be a contiguous fp32 tensor of %d elements" % (name, i, p.numel()))
        e = arr[i]
        e.p, e.g, e.m, e.n, e.lr, e.wd = p.data_ptr(), g.data_ptr(), (m.data_ptr() if m is not None else None), p.numel(), lrs[i], wds[i]
    L, st = lib(), _stream()
    mom, msc = C.c_float(float(momentum)), C.c_float(float(mscale))
    if stats is None:
        check(L.m3d_sgd_step(arr, n, mom, msc, None, None, None, st), "sgd_step")
        return
    _need_gpu(stats)
    if stats.dtype != torch.float64 or stats.numel() != 2 or not stats.is_contiguous():
        raise M3DError("sgd_step: stats must be a contiguous fp64 [2] tensor")
    _bn_ws(lambda ws, nb: L.m3d_sgd_step(arr, n, mom, msc, _ptr(stats), ws, nb, st), stats.device, "sgd_step")


def _step_lists(tag, named, scalars):
    """the argument checks of sgd_step for `named` = ((name, list of tensors or None entries), ...), the first of which gives the sizes,
    and `scalars` = lists with one float per tensor"""
    n = len(named[0][1])
    if not all(len(l) == n for _, l in named) or not all(len(s) == n for s in scalars):
        raise M3DError("%s: %s and the per-tensor scalars must have one entry per tensor" % (tag, ", ".join(k for k, _ in named)))
    for i in range(n):
        p = named[0][1][i]
        for name, l in named:
            t = l[i]
            if t is None and name == "bufs":
                continue
            if not torch.is_tensor(t) or not t.is_cuda:
                raise M3DError("%s: %s[%d] must be a CUDA (ROCm) tensor; there is no CPU path" % (tag, name, i))
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel():
                raise M3DError("%s: %s[%d] must be a contiguous fp32 tensor of %d elements" % (tag, name, i, p.numel()))
    return n


def _step_scalar(tag, name, t, dtype):
    """a device scalar argument (stats fp64 [2], gscale / coef fp32 [1]) -> its pointer, or NULL for None"""
    if t is None:
        return None
    count = 2 if dtype == torch.float64 else 1
    if not torch.is_tensor(t) or not t.is_cuda:
        raise M3DError("%s: %s must be a CUDA (ROCm) tensor; there is no CPU path" % (tag, name))
    if t.dtype != dtype or t.numel() != count or not t.is_contiguous():
        raise M3DError("%s: %s must be a contiguous %s [%d] tensor" % (tag, name, "fp64" if dtype == torch.float64 else "fp32", count))
    return _ptr(t)


def sgd_step_scaled(params, grads, bufs, lrs, wds, momentum, mscale=1.0, stats=None, gscale=None):
    """m3d_sgd_step_scaled: sgd_step with d = s g in front of the decay term, s = gscale, a CUDA fp32 scalar tensor that the kernel reads
    (the coefficient grad_clip_coef wrote); the statistics stay those of the raw gradients.  gscale=None gives the bits of sgd_step."""
    if bufs is None:
        bufs = [None] * len(params)
    n = _step_lists("sgd_step_scaled", (("params", params), ("grads", grads), ("bufs", bufs)), (lrs, wds))
    arr = (SgdTensor * max(n, 1))()
    for i in range(n):
        p, g, m, e = params[i], grads[i], bufs[i], arr[i]
        e.p, e.g, e.m, e.n, e.lr, e.wd = p.data_ptr(), g.data_ptr(), (m.data_ptr() if m is not None else None), p.numel(), lrs[i], wds[i]
    L, st = lib(), _stream()
    mom, msc = C.c_float(float(momentum)), C.c_float(float(mscale))
    gs = _step_scalar("sgd_step_scaled", "gscale", gscale, torch.float32)
    sp = _step_scalar("sgd_step_scaled", "stats", stats, torch.float64)
    if stats is None:
        check(L.m3d_sgd_step_scaled(arr, n, mom, msc, gs, None, None, None, st), "sgd_step_scaled")
        return
    _bn_ws(lambda ws, nb: L.m3d_sgd_step_scaled(arr, n, mom, msc, gs, sp, ws, nb, st), stats.device, "sgd_step_scaled")


def adam_scalars(lr, step, betas):
    """-> (lr_step, bc2_sqrt) of a parameter at its step count `step` (1 at its first step), in Python doubles exactly as the
    single-tensor torch.optim.Adam of this torch forms step_size and bias_correction2_sqrt; m3d_adam_step rounds them to fp32"""
    step = float(step)
    bias_correction1 = 1 - betas[0] ** step
    bias_correction2 = 1 - betas[1] ** step
    return lr / bias_correction1, bias_correction2 ** 0.5


def adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, wds, steps, betas, eps, stats=None, gscale=None):
    """m3d_adam_step: one fused torch.optim.Adam update (amsgrad off, maximize off, coupled weight decay) of a whole parameter list, in
    place and on the current stream.

    params, grads, exp_avgs, exp_avg_sqs: lists of contiguous CUDA fp32 tensors of equal sizes; lrs, wds: one float per tensor; steps:
    each tensor's step count t INCLUDING this step (1 at its first); betas = (beta1, beta2), eps: floats.  Per element d = s g (with
    gscale), d = d + wd p (d where wd == 0), m' = m + (1 - beta1)(d - m), v' = beta2 v + (1 - beta2)(d d), q = sqrt(v') / sqrt(1 -
    beta2^t) + eps, p' = p - lr / (1 - beta1^t) (m' / q), every fp32 operation rounded once.  stats as in sgd_step (of the raw
    gradients); gscale: None, or a CUDA fp32 scalar tensor the kernel reads.  Like sgd_step the update does not bump `_version`."""
    n = _step_lists("adam_step", (("params", params), ("grads", grads), ("exp_avgs", exp_avgs), ("exp_avg_sqs", exp_avg_sqs)),
                    (lrs, wds, steps))
    arr = (AdamTensor * max(n, 1))()
    for i in range(n):
        p, e = params[i], arr[i]
        if not steps[i] >= 1:
            raise M3DError("adam_step: steps[%d] must be at least 1" % i)
        lr_step, bc2_sqrt = adam_scalars(lrs[i], steps[i], betas)
        e.p, e.g, e.m, e.v, e.n = p.data_ptr(), grads[i].data_ptr(), exp_avgs[i].data_ptr(), exp_avg_sqs[i].data_ptr(), p.numel()
        e.lr_step, e.bc2_sqrt, e.wd = lr_step, bc2_sqrt, wds[i]
    L, st = lib(), _stream()
    b1, b2, ep = C.c_double(float(betas[0])), C.c_double(float(betas[1])), C.c_double(float(eps))
    gs = _step_scalar("adam_step", "gscale", gscale, torch.float32)
    sp = _step_scalar("adam_step", "stats", stats, torch.float64)
    if stats is None:
        check(L.m3d_adam_step(arr, n, b1, b2, ep, gs, None, None, None, st), "adam_step")
        return
    _bn_ws(lambda ws, nb: L.m3d_adam_step(arr, n, b1, b2, ep, gs, sp, ws, nb, st), stats.device, "adam_step")


def grad_clip_coef(grads, clip_norm, stats, coef):
    """m3d_grad_clip_coef: one read-only pass over `grads` (contiguous CUDA fp32 tensors) that writes (sum of g^2 in fp64, number of
    non-finite elements) to `stats` (CUDA fp64 [2]) and clip_norm / max(sqrt(sum), clip_norm) to `coef` (CUDA fp32 scalar tensor) - the
    coefficient of the reference's clip_gradient, 1 exactly when the norm does not exceed clip_norm.  Nothing comes back to the host."""
    n = _step_lists("grad_clip_coef", (("grads", grads),), ())
    if stats is None or coef is None:
        raise M3DError("grad_clip_coef: stats and coef are required")
    arr = (GradTensor * max(n, 1))()
    for i in range(n):
        arr[i].g, arr[i].n = grads[i].data_ptr(), grads[i].numel()
    sp = _step_scalar("grad_clip_coef", "stats", stats, torch.float64)
    cp = _step_scalar("grad_clip_coef", "coef", coef, torch.float32)
    L, st, cn = lib(), _stream(), C.c_double(float(clip_norm))
    _bn_ws(lambda ws, nb: L.m3d_grad_clip_coef(arr, n, cn, sp, cp, ws, nb, st), stats.device, "grad_clip_coef")
