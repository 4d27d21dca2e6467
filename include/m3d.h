/* m3d.h — C ABI of libm3d.so: the MI355X (gfx950) implementation of the 3D detection hot path of
 * MeowMeowLady/InstanceSeg-Without-Voxelwise-Labeling.
 *
 * Conventions (all entry points):
 *   - plain C types only; every pointer named d_* is a DEVICE pointer (HBM), caller-allocated;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is asynchronous on it
 *     and never synchronises the device, so calls may be captured into a hipGraph;
 *   - return value: M3D_OK (0) or a negative M3D_E* code; nothing ever calls exit()
 *     (the reference's launchers print and exit(-1): roi_align_kernel_3d.cu:165-169);
 *   - re-entrant; scratch memory comes from the caller (`d_ws`, sized by the matching *_workspace_bytes());
 *     the library never reads the environment and keeps no mutable process-wide state (the tuning knobs below are compiled out of
 *     libm3d.so; they live in the separate tuning build libm3d_tune.so).
 * Paths in comments are relative to the reference repository.
 */
#ifndef M3D_H_
#define M3D_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3D_OK 0
#define M3D_EINVAL (-1)   /* bad argument (shape, NULL pointer, unsupported size) */
#define M3D_ELAUNCH (-2)  /* hipLaunch / runtime error (hipGetLastError) */
#define M3D_EWORKSPACE (-3) /* workspace too small */
#define M3D_EUNSUPPORTED (-4)

int m3d_version(void);
const char* m3d_error_string(int code);
/* Last HIP runtime error text seen by this thread (for M3D_ELAUNCH). */
const char* m3d_last_hip_error(void);
/* Tuning options (benchmark / A-B tooling).  The release library libm3d.so keeps NO mutable process-wide state: there
 * m3d_set_option returns M3D_EUNSUPPORTED for every known name and m3d_get_option reports the built-in defaults.  The knobs are live only
 * in libm3d_tune.so (same objects, m3d_core built with -DM3D_TUNING; m3d_tuning_build() == 1), which the scripts under tools/ and the kernel-family tests load
 * beside the release library.  Names: "xcd_map" (1: XCD-aware workgroup->tile order, default; 0: plain order), "tune_k3", "tune_wino",
 * "tune_wino2_xt" (tile-variant overrides of the conv dispatchers, -1 = library chooses), "tune_wino2" (the 2-D Winograd family behind
 * the default entry points: -1 or 499 = F(2x4,3x3), the library's choice; 299 = F(2x2,3x3); with any other value the
 * m3d_conv3d_wino2_* launches and m3d_conv3d_wino2_plan return M3D_EUNSUPPORTED, the scores and workspace sizes are 0), "tune_fc_slices" /
 * "tune_fc_slices_tail" (split-K factors of m3d_linear_forward), "tune_fc_x3_rows" (128 / 256: tile height of m3d_linear_bf16x3_forward),
 * "tune_fc_x_alias" (> 0: m3d_linear_bf16x3_forward reads row m of x from row m % value - a cache-resident operand, WRONG results:
 * the GEMM's cost with a free operand, tools/f1_ab.py), "tune_stem" (4 / 8: the stem's rows kernel with that many planes per workgroup; any other value: planes by
 * grid size), "tune_fc_x3_rows" = 512 (the 256 x 256 tiles of m3d_linear_f16x2_forward), "tune_roi_xcd" (1: RoIAlign3D's XCD-aware
 * channel split - every XCD one eighth of every RoI's channels; an A/B that removed the L2 misses and not the time, round 6),
 * "tune_zw_grid" (> 0: the m3d_conv3d_zw_* launches start min(value, units) persistent workgroups instead of the library's count, so that
 * each walks more units - the same results bit for bit; for the walk tests and A/B tools, -1 = library chooses).
 * Unknown name -> M3D_EINVAL. */
int m3d_set_option(const char* name, int value);
int m3d_get_option(const char* name, int* value);
int m3d_tuning_build(void);

/* ---------------------------------------------------------------------------------------------------------
 * RoIAlign 3D.  Replaces roi_align_forward_cuda_3d / roi_align_backward_cuda_3d
 * (lib/modeling/roi_xfrom/roi_align_3d/src/roi_align_cuda_3d.h:1-5, .c:7-83; kernels
 * src/roi_align_kernel_3d.cu:81-151, 238-338).
 * features [batch,channels,slices,height,width] fp32; rois [num_rois,roi_cols] fp32, roi_cols must be 7
 * (batch,x1,y1,z1,x2,y2,z2) else M3D_EINVAL (the reference returns 0, roi_align_cuda_3d.c:19-22);
 * output [num_rois,channels,AS,AH,AW] as allocated by functions/roi_align_3d.py:24, written in the
 * reference kernel's (n,c,ph,pw,ps) memory order (roi_align_kernel_3d.cu:87-91).  Caller allocates
 * (and, for backward, zero-fills) the outputs exactly like functions/roi_align_3d.py:24,41-42.
 * ------------------------------------------------------------------------------------------------------- */
int m3d_roi_align3d_forward(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                            int sampling_ratio, const float* d_features, int batch, int channels, int slices,
                            int height, int width, const float* d_rois, int num_rois, int roi_cols,
                            float* d_output, void* stream);
/* Same contract, but every output element is computed in the reference kernel's exact fp32 operation order
 * (8 samples x 8 corner products, roi_align_kernel_3d.cu:73-76,128-147): bit-identical to oracle/m3d_oracle.c.
 * m3d_roi_align3d_forward uses the algebraically equal separable form (three 1-D passes through LDS, ~4x fewer
 * operand reads); the two agree to ~1e-6 * max|feature|. */
int m3d_roi_align3d_forward_exact(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                                  int sampling_ratio, const float* d_features, int batch, int channels, int slices,
                                  int height, int width, const float* d_rois, int num_rois, int roi_cols,
                                  float* d_output, void* stream);
/* m3d_roi_align3d_forward with a caller workspace (m3d_roi_align3d_workspace_bytes(num_rois) bytes, contents irrelevant): the launch takes
 * the RoIs in descending order of their work instead of index order, so the few large RoIs do not form its tail, and the per-RoI set-up
 * (sample tables, folds) is computed once and kept in the workspace instead of once per workgroup.  Identical results. */
size_t m3d_roi_align3d_workspace_bytes(int num_rois);
int m3d_roi_align3d_forward_ws(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                               int sampling_ratio, const float* d_features, int batch, int channels, int slices,
                               int height, int width, const float* d_rois, int num_rois, int roi_cols,
                               float* d_output, void* d_workspace, size_t workspace_bytes, void* stream);
/* Round 6: the same with d_feat_absmax, a device pointer to ONE float >= max |d_features| (m3d_absmax), or NULL (then exactly _ws): RoIs
 * whose sub-volume has <= 128 voxels run as ONE GEMM per RoI on the f16 matrix cores - out[c][bin] = sum_k f[c][k] M[k][bin], M the
 * separable interpolation operator of the RoI, both operands scaled and cut into two fp16 numbers, three products - the others through
 * the separable kernels as before.  Within 1e-6 max |f| of m3d_roi_align3d_forward_ws (the fast mode's contract is 1e-5 max |f|;
 * m3d_roi_align3d_forward_exact stays the reference-order, bit-exact form). */
int m3d_roi_align3d_forward_ws2(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                                int sampling_ratio, const float* d_features, int batch, int channels, int slices,
                                int height, int width, const float* d_rois, int num_rois, int roi_cols,
                                float* d_output, void* d_workspace, size_t workspace_bytes, const float* d_feat_absmax, void* stream);
/* ... and with the bound as feat_absmax_slots floats whose LARGEST is >= max |d_features|: the slot array the conv that produced the
 * feature maps left (m3d_conv3d_zw_forward's d_out_max) instead of a sweep of them; 1 slot is _ws2. */
int m3d_roi_align3d_forward_ws3(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                                int sampling_ratio, const float* d_features, int batch, int channels, int slices, int height,
                                int width, const float* d_rois, int num_rois, int roi_cols, float* d_output, void* d_ws,
                                size_t ws_bytes, const float* d_feat_absmax, int feat_absmax_slots, void* stream);
int m3d_roi_align3d_backward(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                             int sampling_ratio, const float* d_top_grad, const float* d_rois, int num_rois,
                             int roi_cols, float* d_bottom_grad, int batch, int channels, int slices, int height,
                             int width, void* stream);
/* The same gradient in gather form (csrc/roi_align3d_bwd.hip; DESIGN, "RoIAlign3D backward, ordered"): no atomics, EVERY element of
 * d_bottom_grad written exactly once whatever it held (images without a RoI and num_rois == 0 included: zeros, so no zero fill before the
 * call), the result a pure function of (d_top_grad, d_rois, shapes) - bit-identical from call to call, image b's gradient independent of
 * the other images' RoIs.  Same semantics as m3d_roi_align3d_backward; only the order of the fp32 operations differs
 * (|result - exact| <= (n_e + 8) 2^-24 A_e per element, n_e and A_e as in tests/roi_align_backward_cases.py).  Two launches on `stream`, no host synchronisation, allocation or read: graph
 * capturable.  d_workspace: m3d_roi_align3d_backward_ordered_workspace_bytes(num_rois, batch) bytes, 4-byte aligned, contents arbitrary.
 * Returns, before any pointer is followed or anything is launched: M3D_EINVAL for roi_cols != 7, num_rois < 0, a non-positive dimension
 * or bin count, a NULL d_bottom_grad or d_workspace, NULL d_top_grad / d_rois with num_rois > 0, a workspace that is too small;
 * M3D_EUNSUPPORTED for a fixed sampling_ratio with bins * sampling_ratio > 64 on an axis (the rule of m3d_roi_align3d_backward) and for
 * more than 64 bins on an axis.  An ADAPTIVE grid (sampling_ratio <= 0) that needs more than 64 table entries on an axis of ANY RoI is
 * found on the device: the call then writes NOTHING to d_bottom_grad and leaves 1 in the first int32 of d_workspace (0 otherwise); the
 * caller reads that word after the stream has reached it (m3d.ops.roi_align3d_backward_ordered does, and raises).  With a fixed ratio the
 * word is always 0 and need not be read. */
size_t m3d_roi_align3d_backward_ordered_workspace_bytes(int num_rois, int batch);
int m3d_roi_align3d_backward_ordered(int aligned_slices, int aligned_height, int aligned_width, float spatial_scale,
                                     int sampling_ratio, const float* d_top_grad, const float* d_rois, int num_rois,
                                     int roi_cols, float* d_bottom_grad, int batch, int channels, int slices, int height,
                                     int width, void* d_workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Greedy 3D NMS.  Replaces utils.cython_nms_3d.nms_3d / nms_3d_volume
 * (lib/utils/cython_nms_3d.pyx:39-96, 102-159; wrappers lib/utils/boxes_3d.py:364-374).
 * d_dets [n,7] fp32 rows (x1,y1,z1,x2,y2,z2,score).  Visiting order: descending score (by_volume=0) or
 * descending volume (by_volume=1), ties in descending input index.  d_keep receives the surviving INPUT
 * indices in ascending order (np.where(suppressed == 0)[0], pyx:96); *d_num_keep their count.
 * fp32 arithmetic, `ovr >= thresh`, bit-exact with the reference.
 * n <= 16384: rank sort, N x N/64 IoU bitmask, one workgroup resolves it from LDS.  16384 < n <= 2^20 (round 6; the cross-tile NMS of
 * a whole volume's detections - tools/binarization_nuclei.py:81, tools/binarization_soma.py:57, lib/core/test.py:159 - has no bound in
 * the reference): the blocked form - chunks of 1024 sorted rows, a chunk's own 1024 x 1024 bitmask resolved by one workgroup against
 * the global removed bitmap, its kept boxes then tested against every later live box by a wide launch; same result, O(kept x alive)
 * IoUs, workspace n x 176 bytes.  n > 2^20: M3D_EUNSUPPORTED (the O(n^2) rank sort alone would take seconds).
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_nms3d_workspace_bytes(int n);
int m3d_nms3d(const float* d_dets, int n, float thresh, int by_volume, int64_t* d_keep, int32_t* d_num_keep,
              void* d_ws, size_t ws_bytes, void* stream);

/* N x K IoU matrix.  Replaces utils.cython_bbox_3d.bbox_overlaps_3d (lib/utils/cython_bbox_3d.pyx:32-80).
 * d_boxes [n,6], d_query [k,6] fp32 -> d_out [n,k] fp32 (fp32 intersection, fp64 union and divide). */
int m3d_bbox_overlaps3d(const float* d_boxes, int n, const float* d_query, int k, float* d_out, void* stream);

/* Box decode + clip.  Replaces utils.boxes_3d.bbox_transform_3d / clip_tiled_boxes_3d
 * (lib/utils/boxes_3d.py:167-225, 144-163).  d_boxes [n,6] fp32, d_deltas [n,6*classes] fp32,
 * weights[6] host doubles, xform_clip = cfg.BBOX_XFORM_CLIP; d_out [n,6*classes].
 * If clip_slices > 0 the result is also clipped to [0,dim-1] (x:width, y:height, z:slices). */
int m3d_bbox_transform3d(const float* d_boxes, const float* d_deltas, int n, int classes, const double* weights,
                         double xform_clip, double clip_slices, double clip_height, double clip_width,
                         float* d_out, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * RPN proposal generation for one image, fully on device.  Replaces GenerateProposalsOp_3d.forward /
 * proposals_for_one_image / _filter_boxes_3d (lib/modeling/generate_proposals_3d.py:19-192), which in the
 * reference copies scores and deltas to the host (:58-63).
 * d_scores [A,S,H,W] fp32 (post-sigmoid), d_deltas [6A,S,H,W] fp32, anchors[A*6] host doubles
 * (generate_anchors_3d), im_info = (slices,height,width,scale) host doubles.
 * Outputs (capacity post_nms_topN, or pre_nms_topN when post <= 0): d_rois [R,7] fp32 (batch column =
 * batch_index), d_probs [R] fp32, d_keep_idx [R] int64 = flat index into (S,H,W,A) (:160,174-175),
 * *d_num = R.  Top-N tie rule: descending score, ties ascending flat index.
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_generate_proposals3d_workspace_bytes(int A, int S, int H, int W, int pre_nms_topN);
int m3d_generate_proposals3d(const float* d_scores, const float* d_deltas, int A, int S, int H, int W,
                             const double* anchors, double feat_stride, const double* im_info,
                             int pre_nms_topN, int post_nms_topN, float nms_thresh, double min_size,
                             double xform_clip, int batch_index, float* d_rois, float* d_probs,
                             int64_t* d_keep_idx, int32_t* d_num, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * 3D convolution (cross-correlation), NCDHW fp32, stride 1, zero padding k/2, dilation 1, groups 1 — what
 * torch.nn.Conv3d computes for every conv of lib/modeling/DSN.py:19-36 and lib/modeling/rpn_heads.py:54-61.
 * fp32 MFMA (v_mfma_f32_32x32x2_f32) implicit GEMM, LDS-staged halo tiles, no im2col buffer.
 *
 * Weights are packed once (m3d_conv3d_pack_weights) into the MFMA A-fragment order; `mode` selects
 *   M3D_W_PLAIN     W                       (forward conv)
 *   M3D_W_RELU      relu(W)                 (PRM norm conv, lib/prm/peak_backprop_3d.py:41-42)
 *   M3D_W_DGRAD     flip + transpose W      (backward-data of a stride-1 same conv)
 *   M3D_W_DGRAD_RELU flip + transpose relu(W) (PRM backward, peak_backprop_3d.py:16-18 via autograd)
 * Forward computes, per output element:  y = conv(x - in_offset, Wp) ; y = y*scale[c] + shift[c] (if given;
 * bias and eval-mode BatchNorm fold into scale/shift) ; y = max(y,0) (if relu) ; y *= mul[..] (if d_mul given:
 * same shape as the output; the PRM PreHook product).  Padding voxels stay 0 after the offset subtraction.
 * ------------------------------------------------------------------------------------------------------- */
enum { M3D_W_PLAIN = 0, M3D_W_RELU = 1, M3D_W_DGRAD = 2, M3D_W_DGRAD_RELU = 3 };
size_t m3d_conv3d_packed_weight_bytes(int cin, int cout, int k, int mode);
int m3d_conv3d_pack_weights(const float* d_weight /*[cout,cin,k,k,k]*/, int cin, int cout, int k, int mode,
                            float* d_packed, void* stream);
int m3d_conv3d_forward(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                       int depth, int height, int width, int k, const float* d_in_offset /*1 float or NULL*/,
                       const float* d_scale, const float* d_shift, int relu, const float* d_mul, void* stream);
/* The two 1x1x1 RPN heads as ONE convolution with both epilogues (lib/modeling/rpn_heads.py:96-98 and the sigmoid of :116): output
 * channels [0, split) -> 1 / (1 + exp(-v)) -> d_out_sigmoid [batch, split, D, H, W]; channels [split, cout) -> d_out_rest
 * [batch, cout - split, D, H, W].  d_packed = m3d_conv3d_pack_weights of the concatenated weights; d_shift = the concatenated biases. */
int m3d_conv3d_forward_split_sigmoid(const float* d_in, const float* d_packed, float* d_out_sigmoid, float* d_out_rest, int batch, int cin,
                                     int cout, int split, int depth, int height, int width, int k, const float* d_shift, void* stream);
/* 3x3x3 "same" convolution with dilation 2 / padding 2 (dilation 1 = m3d_conv3d_forward): the convolutions of the mask head
 * (lib/modeling/mask_rcnn_heads.py:148-151 with MRCNN.DILATION = 2, lib/core/config.py:767).  d_packed: m3d_conv3d_pack_weights.
 * With the M3D_W_DGRAD pack of a layer's weights, that layer's output gradient as d_in, cin and cout exchanged and d_scale = d_shift =
 * NULL, relu = 0 it is the layer's backward-data (padding = dilation makes the transposed conv the same dilated conv of the flipped,
 * transposed weights).  k = 3 and dilation 2 only; any other (k, dilation > 1) is M3D_EUNSUPPORTED. */
int m3d_conv3d_forward_dilated(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout, int depth,
                               int height, int width, int k, int dilation, const float* d_scale, const float* d_shift, int relu,
                               void* stream);

/* Which instantiation of the direct kernel m3d_conv3d_forward (pool = 0; also _windowed and _split_sigmoid) or m3d_conv3d_forward_pool2
 * (pool = 1) launches for this shape: a dense id in [0, m3d_conv3d_direct_plan_count()), the input channels it stages per chunk (1 for the
 * 5^3 stem, whose K index is the tap), its voxel tile, the 32-channel output blocks per workgroup and its in-workgroup K split (1 or 2).
 * Host only, no device call; returns exactly what the launch would return before launching (M3D_EUNSUPPORTED / M3D_EINVAL, outputs then
 * untouched); any output pointer may be NULL.  The "tune_k3" option of the tuning build overrides the launch, not this answer. */
int m3d_conv3d_direct_plan(int batch, int cin, int cout, int depth, int height, int width, int k, int pool, int* variant, int* cc,
                           int* tile_x, int* tile_y, int* tile_z, int* ncb, int* ksplit);
int m3d_conv3d_direct_plan_count(void);

/* 3x3x3 forward convolution with the Winograd F(2,3) transform along x (csrc/conv3d_wino.hip): the same operation as
 * m3d_conv3d_forward for k = 3, plain weights, no input offset / PRM multiply, at 2/3 of the MFMA work.  Results
 * agree with the direct kernel to a few fp32 ulp (tolerance of this path: 1e-4 relative, north_star), not bit for
 * bit, so the PRM norm / backward convolutions never use it.  Own packed-weight layout (36 slots per cout x cin).
 * Returns M3D_EUNSUPPORTED for maps narrower than 24 voxels (callers then use m3d_conv3d_forward). */
size_t m3d_conv3d_wino_packed_weight_bytes(int cin, int cout);
int m3d_conv3d_wino_pack_weights(const float* d_weight /*[cout,cin,3,3,3]*/, int cin, int cout, float* d_packed,
                                 void* stream);
int m3d_conv3d_wino_forward(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                            int depth, int height, int width, const float* d_scale, const float* d_shift, int relu,
                            void* stream);
/* the same fused with MaxPool3d(2,2) (DSN.py:60-61): writes [batch,cout,D/2,H/2,W/2]; width >= 48 */
int m3d_conv3d_wino_forward_pool2(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                                  int depth, int height, int width, const float* d_scale, const float* d_shift,
                                  int relu, void* stream);

/* The same with Winograd F(2x2,3x3) on the (y,x) plane (csrc/conv3d_wino2.hip): 4/9 of the MFMA work; own packed layout
 * (48 slots per cout x cin); maps >= 24 wide, fused pool >= 48 wide; same few-ulp agreement with the direct kernel. */
size_t m3d_conv3d_wino2_packed_weight_bytes(int cin, int cout);
int m3d_conv3d_wino2_pack_weights(const float* d_weight /*[cout,cin,3,3,3]*/, int cin, int cout, float* d_packed,
                                  void* stream);
int m3d_conv3d_wino2_forward(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                             int depth, int height, int width, const float* d_scale, const float* d_shift, int relu,
                             void* stream);
/* small maps (12..23 voxels wide, e.g. the 16^3 stage-4 layers): 16x16x2 output tiles with split-K over workgroups;
 * partial results go to the caller's workspace and are summed in a fixed order by a second kernel (deterministic).
 * m3d_conv3d_wino2_forward_ws dispatches to m3d_conv3d_wino2_forward for maps >= 24 wide (workspace unused). */
size_t m3d_conv3d_wino2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width);
/* useful-work x chip-fill score (0..1) of the tile the library would pick (64x2x4, 32x8x2 or 16x16x2 with split-K);
 * below ~0.5 the direct kernel is the better choice */
double m3d_conv3d_wino2_score(int batch, int cin, int cout, int depth, int height, int width);
/* ... and for the exactly-local F(2x2,3x3) family of m3d_conv3d_wino2_local_forward_ws (other tiles, hence its own score) */
double m3d_conv3d_wino2_local_score(int batch, int cin, int cout, int depth, int height, int width);
/* the 2-D Winograd kernel family behind the default entry points: 4 = F(2x4,3x3) (F(2,3) along y, F(4,3) along x: 1/3 of the direct
 * convolution's multiplies; the release library always), 2 = F(2x2,3x3) (4/9; the family of the "_local" entry points, here only
 * under option "tune_wino2" = 299 of the tuning build), 0 = that option holds a value that names no family */
int m3d_conv3d_wino2_family(void);
/* What m3d_conv3d_wino2_forward_ws (local = 0) / m3d_conv3d_wino2_local_forward_ws (local = 1) would launch for this shape: kernel
 * family, tile id (32 / 16 / 8; 0: none) and K split (1: one accumulation chain per output over the input channels; s > 1: s partial
 * sums added in a fixed order, i.e. another summation order).  A pure function of the shape - no launch, no device access; replaces
 * nothing in the reference (cuDNN's algorithm choice behind `F.conv3d`, lib/prm/peak_backprop_3d.py:40-42, is equally shape-dependent). */
int m3d_conv3d_wino2_plan(int local, int batch, int cin, int cout, int depth, int height, int width, int* family_out, int* tile_out,
                          int* ksplit_out);
int m3d_conv3d_wino2_forward_ws(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                                int depth, int height, int width, const float* d_scale, const float* d_shift, int relu,
                                void* d_ws, size_t ws_bytes, void* stream);
/* The same forward through the F(2x2,3x3) family only, whose outputs depend on nothing outside their own 3 x 3 (y, x) support, not
 * even by rounding (the default family's F(4,3) along x cancels the rest of its 6-wide footprint only to ~1e-7 of those inputs).
 * Used where unrelated data sits right next to a window (the PRM strip layout, m3d_prm_prepare_ex). */
size_t m3d_conv3d_wino2_local_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width);
int m3d_conv3d_wino2_local_forward_ws(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                                      int depth, int height, int width, const float* d_scale, const float* d_shift, int relu,
                                      void* d_ws, size_t ws_bytes, void* stream);
int m3d_conv3d_wino2_forward_pool2(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                                   int depth, int height, int width, const float* d_scale, const float* d_shift,
                                   int relu, void* stream);
/* the same with the pool's argmax (uint8 [batch, cout, D/2, H/2, W/2], dz*4 + dy*2 + dx of the first maximum: the rule of
 * m3d_maxpool3d_2x_forward) - the response conv of the pooled layers in PRM mode */
int m3d_conv3d_wino2_forward_pool2_argmax(const float* d_in, const float* d_packed, float* d_out, unsigned char* d_argmax, int batch,
                                          int cin, int cout, int depth, int height, int width, const float* d_scale,
                                          const float* d_shift, int relu, void* stream);

/* conv1a (5x5x5, one input channel; DSN.py:19,58) with Winograd F(2,5) along x (csrc/conv3d_stem_wino.hip): 0.62x the MFMA
 * work of the direct stem kernel; own packed layout; pool != 0 fuses MaxPool3d(2,2) and writes [batch,cout,D/2,H/2,W/2].
 * Maps >= 32 voxels wide; agreement with the direct kernel ~1e-6 relative to the tensor maximum. */
size_t m3d_conv3d_stem_wino_packed_weight_bytes(int cout);
int m3d_conv3d_stem_wino_pack_weights(const float* d_weight /*[cout,1,5,5,5]*/, int cout, float* d_packed, void* stream);
int m3d_conv3d_stem_wino_forward(const float* d_in, const float* d_packed, float* d_out, int batch, int cout, int depth,
                                 int height, int width, const float* d_scale, const float* d_shift, int relu, int pool,
                                 void* stream);
/* Round 6: the same launch also leaves the largest |output| in d_out_max (32 floats, zeroed by the caller, atomic maxima; NULL: exactly
 * the call above) - the operand bound m3d_conv3d_zw_forward takes as d_in_max, so that the layer behind the stem needs no sweep. */
int m3d_conv3d_stem_wino_forward_bound(const float* d_in, const float* d_packed, float* d_out, int batch, int cout, int depth,
                                       int height, int width, const float* d_scale, const float* d_shift, int relu, int pool,
                                       float* d_out_max, void* stream);
/* What the two calls above would launch for this shape: the planes per workgroup of the rows kernel (4, or 8 from a grid that fills
 * the chip four times over), from the launch's own decision, and the launch's own refusals.  Host only: no launch, no device access. */
int m3d_conv3d_stem_wino_plan(int batch, int cout, int depth, int height, int width, int pool, int* planes_out);

/* Backward-weights and bias gradient of the same stride-1 "same" convolution (what autograd computes for the
 * F.conv3d calls of lib/prm/peak_backprop_3d.py:40-42 and every nn.Conv3d of lib/modeling/DSN.py:19-36 in training):
 *   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+dz-k/2,...]     db[co] = sum gy[b,co,...]
 * fp32 MFMA implicit GEMM with the voxel index as the reduction dimension; split-K partials go to the workspace and
 * are summed in a fixed order (deterministic).  k = 1, 3 any cin; k = 5 with cin = 1.  d_grad_weight is [cout,cin,k,k,k]. */
size_t m3d_conv3d_wgrad_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k);
int m3d_conv3d_wgrad(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                     int depth, int height, int width, int k, void* d_ws, size_t ws_bytes, void* stream);
int m3d_conv3d_bias_grad(const float* d_grad_out, float* d_grad_bias, int batch, int cout, int depth, int height,
                         int width, void* stream);
/* Backward-weights of the dilated "same" convolution of m3d_conv3d_forward_dilated (padding = dilation): what autograd computes for the
 * nn.Conv3d(dim, dim, 3, 1, padding=d, dilation=d) layers of lib/modeling/mask_rcnn_heads.py:141-151 with MRCNN.DILATION = d in training:
 *   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci, z+d(dz-1), y+d(dy-1), x+d(dx-1)]          (zero outside the volume)
 *   dilation 1     m3d_conv3d_wgrad / m3d_conv3d_wgrad_workspace_bytes with the same arguments: bit-equal, every k it takes.
 *   k 3, dilation 2  csrc/conv3d_wgrad.hip: the fp32 MFMA implicit GEMM of m3d_conv3d_wgrad (v_mfma_f32_32x32x2_f32, fp32
 *                  operands and accumulation) on a voxel tile with a 2-voxel halo: 2 x 8 x 8 for maps at most 8 wide (the 7^3 RoI
 *                  grid), 2 x 4 x 16 beyond.  `slots` split-K partials (a function of the shape only, m3d_conv3d_wgrad_dilated_plan)
 *                  go to the workspace; a reduce launch adds them in slot order.  No atomics: bit-identical run to run.  Writes every
 *                  element of d_grad_weight [cout,cin,3,3,3] and at most workspace_bytes of d_ws, nothing else.
 * Refusals, all before a pointer is followed or anything is launched (so with any non-NULL pointers on a machine without a GPU):
 * M3D_EINVAL a NULL pointer or a non-positive extent; M3D_EUNSUPPORTED any other (k, dilation), cin or cout * depth * height * width
 * * 4 bytes >= 2^31 - 1 (one image is addressed with 32-bit offsets), 2^31 voxel tiles or workgroups (workspace_bytes is then 0);
 * M3D_EWORKSPACE ws_bytes below workspace_bytes.
 * Backward-data needs no entry point of its own: with padding = dilation, gx is m3d_conv3d_forward_dilated of gy on the M3D_W_DGRAD
 * pack (cin and cout exchanged, d_scale = d_shift = NULL, relu = 0).
 * m3d_conv3d_wgrad_dilated_tile (dilation 2 only; dilation 1 is M3D_EUNSUPPORTED): the same with the tile's x extent chosen by the
 * caller (16: 2 x 4 x 16, 8: 2 x 8 x 8, 0: the library's choice; anything else M3D_EUNSUPPORTED) on the same workspace - the A/B tool
 * and the tests of both forms.  _plan (host only; any output pointer may be NULL; dilation 2 only) reports the tile and the slot
 * count of such a call and returns what it would return for its shape. */
size_t m3d_conv3d_wgrad_dilated_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k, int dilation);
int m3d_conv3d_wgrad_dilated(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout, int depth,
                             int height, int width, int k, int dilation, void* d_ws, size_t ws_bytes, void* stream);
int m3d_conv3d_wgrad_dilated_tile(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                  int depth, int height, int width, int k, int dilation, int tile_x, void* d_ws, size_t ws_bytes,
                                  void* stream);
int m3d_conv3d_wgrad_dilated_plan(int batch, int cin, int cout, int depth, int height, int width, int k, int dilation, int tile_x,
                                  int* tile_x_out, int* tile_y_out, int* slots_out);
/* The k = 3, dilation 1 weight gradient of m3d_conv3d_wgrad on maps at most 8 voxels wide (csrc/conv3d_wgrad.hip): the per-RoI
 * convs on 7^3 grids of lib/modeling/fast_rcnn_heads.py:120-179 (roi_Xconv1fc_head) and of the mask head at MRCNN.DILATION = 1.  The
 * scheme of the dilated kernel above (v_mfma_f32_32x32x2_f32, fp32 operands and accumulation, `slots` split-K partials in the
 * workspace, a reduce launch that adds them in slot order; no atomics: bit-identical run to run) on a 2 x 8 x 8 voxel tile with a
 * 1-voxel halo, where m3d_conv3d_wgrad has only 2 x 4 x 16.  Same sum as m3d_conv3d_wgrad in another order: equal within fp32
 * rounding, not bit-equal.  Writes every element of d_grad_weight [cout,cin,3,3,3] and at most workspace_bytes of d_ws, nothing else.
 * Refusals, all before a pointer is followed or anything is launched: M3D_EINVAL a NULL pointer or a non-positive extent;
 * M3D_EUNSUPPORTED k != 3, width > 8, cin or cout * depth * height * width * 4 bytes >= 2^31 - 1, 2^31 voxel tiles or workgroups
 * (workspace_bytes is then 0 and _supported 0); M3D_EWORKSPACE ws_bytes below workspace_bytes.
 * _plan (host only; any output pointer may be NULL) reports the tile (8, 8) and the slot count, a function of the shape only, and
 * returns what the launch would return for its shape. */
int m3d_conv3d_wgrad_narrow_supported(int batch, int cin, int cout, int depth, int height, int width, int k);
size_t m3d_conv3d_wgrad_narrow_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width, int k);
int m3d_conv3d_wgrad_narrow_plan(int batch, int cin, int cout, int depth, int height, int width, int k, int* tile_x_out,
                                 int* tile_y_out, int* slots_out);
int m3d_conv3d_wgrad_narrow(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout, int depth,
                            int height, int width, int k, void* d_ws, size_t ws_bytes, void* stream);
/* The k = 3 weight gradient above on the f16 matrix cores at fp32 accuracy (csrc/conv3d_wgrad_f16.hip): the f16x2 cut of
 * m3d_conv3d_zw_forward - each operand tensor scaled by ONE power of two (m3d::f16_scale_of of its bound) and cut into two fp16
 * numbers while it is staged, three v_mfma_f32_32x32x16_f16 products hh + hl + lh per fp32 product, fp32 accumulation, the sum
 * multiplied by 1 / s_g and 1 / s_x once at the end (exact).  d_in_max / d_gy_max: device arrays of m3d_conv3d_zw_slots() non-negative
 * floats whose LARGEST is >= max |d_in| / max |d_grad_out| (what m3d_conv3d_zw_forward leaves in d_out_max; m3d_conv3d_zw_bound_of
 * sweeps a tensor).  An input beyond its bound overflows fp16 (inf / NaN): the caller's contract, as for the zw forward.
 *   supported   cin and cout multiples of 32 (<= 4096), every extent >= 1, at most 2^30 voxel tiles of 2 x 4 x 16 and (2^32 - 1) / 192
 *               workgroups (a launch of fewer than 2^32 threads); everything else (and k != 3) stays on m3d_conv3d_wgrad.
 *   accumulation  no accumulator takes more than `chain` <= 384 consecutive MFMAs (the f16 MFMA truncates when it adds): a split-K slot
 *               is `tiles_per_slot` <= 16 tiles (24 MFMAs per accumulator and tile) and writes its partial to the workspace; the reduce
 *               launch adds the `slots` partials with fp32 round-to-nearest adds in a fixed order (8 strided groups, then the 8 group
 *               sums in order).  slots and tiles_per_slot are functions of the shape only; no atomics: bit-identical run to run and
 *               from stream to stream.  m3d_conv3d_wgrad_f16x2_plan (host only; any output pointer may be NULL) reports them: `chain`
 *               the longest MFMA chain of an accumulator, `folds` the fp32 operations behind it on the longest path of an output
 *               (ceil(slots / 8) + 7 adds, 2 scale multiplies).
 *   zeros       an all-zero operand (bound 0) gives an exactly zero gradient; an output none of whose products is non-zero is exactly 0
 *               (the cut of 0 is 0 and voxels outside the volume are staged as zeros).
 *   writes      d_grad_weight [cout,cin,3,3,3] and slots * cout * cin * 27 floats of d_ws (workspace_bytes; 16-byte aligned), nothing else.
 * Refusals, before any pointer is followed or anything is launched.  M3D_EINVAL: a NULL pointer, a float pointer that is not 4-byte
 * aligned, a d_ws that is not 16-byte aligned, a non-positive extent, ws_bytes below workspace_bytes.  M3D_EUNSUPPORTED: whatever
 * `supported` rejects (workspace_bytes is then 0). */
int m3d_conv3d_wgrad_f16x2_supported(int batch, int cin, int cout, int depth, int height, int width);
size_t m3d_conv3d_wgrad_f16x2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width);
int m3d_conv3d_wgrad_f16x2_plan(int batch, int cin, int cout, int depth, int height, int width, int* slots, int* tiles_per_slot,
                                int* chain, int* folds);
int m3d_conv3d_wgrad_f16x2(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout, int depth,
                           int height, int width, const float* d_in_max, const float* d_gy_max, void* d_ws, size_t ws_bytes,
                           void* stream);
/* m3d_conv3d_wgrad_f16x2 for maps at most 8 voxels wide (csrc/conv3d_wgrad_narrow_f16.hip): the same cut, contract, argument order and
 * refusals, on the 2 x 8 x 8 voxel tile of m3d_conv3d_wgrad_narrow (a 7^3 RoI grid fills 343 of its 512 slots, 343 of 1024 of the
 * wide kernel's).  A 16-deep k-step is two 8-voxel rows; the +-1 shift along x is built in registers with a zero shifted in, since
 * x = -1 and x = 8 are outside every map this kernel takes.  M3D_EUNSUPPORTED: width > 8, cin or cout not a multiple of 32 or above
 * 4096, too many workgroups.  _plan also reports tile_z, the tile's depth (the tile is tile_z x 8 x 8): chain = tiles_per_slot *
 * (tile_z * 8 / 2) * 3 <= 384, folds = ceil(slots / 8) + 7 adds + 2 scale multiplies.  workspace_bytes = slots * 27 * cin * cout * 4. */
int m3d_conv3d_wgrad_narrow_f16x2_supported(int batch, int cin, int cout, int depth, int height, int width);
size_t m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width);
int m3d_conv3d_wgrad_narrow_f16x2_plan(int batch, int cin, int cout, int depth, int height, int width, int* tile_z, int* slots,
                                       int* tiles_per_slot, int* chain, int* folds);
int m3d_conv3d_wgrad_narrow_f16x2(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                  int depth, int height, int width, const float* d_in_max, const float* d_gy_max, void* d_ws,
                                  size_t ws_bytes, void* stream);
/* m3d_conv3d_wgrad_narrow_f16x2 with a dilation (the second instantiation of the same kernel): `dilation` 1 is that call, bit for bit;
 * `dilation` 2 is the weight gradient of the k = 3, dilation 2, padding 2 convs (the mask head at MRCNN.DILATION = 2 on 7^3 RoI grids),
 *   dW[co,ci,dz,dy,dx] = sum_{b,z,y,x} gy[b,co,z,y,x] * x[b,ci,z+2(dz-1),y+2(dy-1),x+2(dx-1)]   (zeros outside the map)
 * with the same cut, contract, tile, slot rule and reduce launch.  The halo image of x grows to 6 x 12 rows (92,160 bytes of LDS, one
 * workgroup per CU); the +-2 shift along x is a move of whole dwords in registers with a zero dword shifted in, since x = -2, -1, 8 and
 * 9 are outside every map this kernel takes.  The number of MFMAs per tile does not depend on the dilation: _plan reports the tile_z,
 * slots, tiles_per_slot, chain and folds of m3d_conv3d_wgrad_narrow_f16x2_plan for the same shape, and workspace_bytes is the same
 * slots * 27 * cin * cout * 4.
 *   supported   dilation 1 or 2 and what m3d_conv3d_wgrad_narrow_f16x2_supported takes (width <= 8, cin and cout multiples of 32 and at
 *               most 4096, the same tile-count and workgroup-count limits).  Any other dilation is unsupported (workspace_bytes 0).
 * Refusals, before any pointer is followed or anything is launched, in the order of the dilation-1 entry.  M3D_EINVAL: a NULL pointer, a
 * float pointer that is not 4-byte aligned, a d_ws that is not 16-byte aligned, a non-positive extent, dilation < 1, ws_bytes below
 * workspace_bytes.  M3D_EUNSUPPORTED: whatever `supported` rejects, dilation > 2 among it. */
int m3d_conv3d_wgrad_narrow_dilated_f16x2_supported(int batch, int cin, int cout, int depth, int height, int width, int dilation);
size_t m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width,
                                                             int dilation);
int m3d_conv3d_wgrad_narrow_dilated_f16x2_plan(int batch, int cin, int cout, int depth, int height, int width, int dilation, int* tile_z,
                                               int* slots, int* tiles_per_slot, int* chain, int* folds);
int m3d_conv3d_wgrad_narrow_dilated_f16x2(const float* d_in, const float* d_grad_out, float* d_grad_weight, int batch, int cin, int cout,
                                          int depth, int height, int width, int dilation, const float* d_in_max, const float* d_gy_max,
                                          void* d_ws, size_t ws_bytes, void* stream);
/* One pass over a conv layer's output gradient d_gy [batch, cout, depth, height, width] (csrc/conv3d_gy_reduce.hip) for the bias gradient
 * and the operand bound the f16x2 dgrad (m3d_conv3d_zw_forward on an m3d_conv3d_zw_pack_dgrad pack) and m3d_conv3d_wgrad_f16x2 take:
 *   d_grad_bias  (or NULL) [cout]: gb[c] = fp32(S), S = the sum of d_gy[:, c] taken in fp64 over spans of one (image, channel) slab whose
 *                boundaries depend on the shape only, a fixed order inside a span and an ascending (image, span) loop over a channel's
 *                partials; one rounding to fp32.  No floating-point atomics: bit-identical run to run and stream to stream.
 *                |gb - S_exact| <= 2^-24 |S_exact| + n 2^-53 sum |gy|, n = batch depth height width.
 *   d_gy_max     m3d_conv3d_zw_slots() floats, written here (no need to zero them): the LARGEST equals max |d_gy| exactly (what
 *                m3d_conv3d_zw_bound_of gives); a non-finite value in d_gy makes it non-finite.
 * Workspace: the convention of m3d_bn_*: with d_ws == NULL the call launches nothing and stores the bytes it needs in *ws_bytes; otherwise
 * *ws_bytes is the capacity of d_ws (8-byte aligned; M3D_EWORKSPACE if too small).  Refusals, before any pointer is followed: M3D_EINVAL for
 * a non-positive extent, a NULL or misaligned d_gy / d_gy_max, a misaligned d_grad_bias, a NULL ws_bytes; M3D_EUNSUPPORTED for a slab of 2^31
 * elements or more, or 2^24 spans (16384 elements of one slab each) or more. */
int m3d_conv3d_gy_reduce(const float* d_gy, int batch, int cout, int depth, int height, int width, float* d_grad_bias, float* d_gy_max,
                         void* d_ws, size_t* ws_bytes, void* stream);

/* Conv + scale/shift + ReLU + MaxPool3d(2,2) fused (DSN.py:58,60-61: pool1/pool2 directly follow a conv):
 * writes only the pooled tensor [batch,cout,D/2,H/2,W/2] (8x fewer output bytes, no separate pool pass) and,
 * if d_argmax != NULL, the window index (z*4+y*2+x, first maximum) for the PRM un-pooling.  Supported for the
 * 5^3 stem (cout <= 32) and k = 3 with width >= 24; otherwise M3D_EUNSUPPORTED (use conv + m3d_maxpool3d_2x). */
int m3d_conv3d_forward_pool2(const float* d_in, const float* d_packed, float* d_out_pooled, uint8_t* d_argmax,
                             int batch, int cin, int cout, int depth, int height, int width, int k,
                             const float* d_in_offset, const float* d_scale, const float* d_shift, int relu,
                             void* stream);

/* Same conv on a batch of cropped windows, with the PRM PreHook multiply fused: out[b,co,z,y,x] *=
 * full[co, origin_b + (z,y,x)] - *d_full_offset, and 0 where that position lies outside the full tensor
 * (lib/prm/peak_backprop_3d.py:16-18 restricted to each peak's receptive-field cone).
 * d_full [cout, full_depth, full_height, full_width]; d_origins int32 [batch,3] = (z,y,x) of each window. */
int m3d_conv3d_forward_windowed(const float* d_in, const float* d_packed, float* d_out, int batch, int cin, int cout,
                                int depth, int height, int width, int k, const float* d_full,
                                const float* d_full_offset, const int32_t* d_origins, int full_depth,
                                int full_height, int full_width, void* stream);

/* MaxPool3d(kernel 2, stride 2, floor) forward with argmax (lib/modeling/DSN.py:21,26,32) and its
 * backward (gradient routed to the argmax voxel; first maximum in z,y,x scan order wins, as PyTorch). */
int m3d_maxpool3d_2x_forward(const float* d_in, float* d_out, uint8_t* d_argmax /*may be NULL*/, int batch_channels,
                             int depth, int height, int width, void* stream);
int m3d_maxpool3d_2x_backward(const float* d_grad_out, const uint8_t* d_argmax, float* d_grad_in,
                              int batch_channels, int depth, int height, int width, void* stream);

/* Global minimum of a device fp32 array into d_out[0] (the `input.min()` offset of
 * lib/prm/peak_backprop_3d.py:38); stays on device so the PRM convs never synchronise with the host. */
size_t m3d_reduce_min_workspace_bytes(void);
int m3d_reduce_min(const float* d_in, int64_t n, float* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* The minima of up to 12 arrays in two launches (the PRM forward: one `input.min()` per patched conv): d_ins / counts are HOST arrays of
 * `count` device pointers / element counts, d_out [count] on the device. */
size_t m3d_reduce_min_multi_workspace_bytes(void);
int m3d_reduce_min_multi(const float* const* d_ins, const int64_t* counts, int count, float* d_out, void* d_ws, size_t ws_bytes,
                         void* stream);
/* Round 6: minima AND maxima of the same arrays in the same two launches (d_mins / d_maxs [count]); workspace
 * m3d_reduce_minmax_multi_workspace_bytes().  The f16x2 norm convolutions (m3d_conv3d_x3f_forward_ws) scale X - min X by max X - min X. */
size_t m3d_reduce_minmax_multi_workspace_bytes(void);
int m3d_reduce_minmax_multi(const float* const* d_ins, const int64_t* counts, int count, float* d_mins, float* d_maxs, void* d_ws,
                            size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Batched, fused box post-processing: ONE launch per stage for a whole batch of tiles, one workgroup per tile, no host
 * round trips (csrc/box_fused.hip).  Same results as the per-tile entry points above, item by item.  Every item may
 * hold at most m3d_fused_max_boxes() (2048) boxes, else M3D_EUNSUPPORTED (use the per-tile entry points).
 *   m3d_generate_proposals3d_batched  GenerateProposalsOp_3d.forward (lib/modeling/generate_proposals_3d.py:19-192) for
 *       d_scores [batch,A,S,H,W] / d_deltas [batch,6A,S,H,W]: outputs d_rois [batch,out_rows,7] (column 0 =
 *       first_batch_index + item), d_probs [batch,out_rows], d_keep_idx [batch,out_rows], d_num [batch].
 *   m3d_box_results3d_batched         box_results_with_nms_and_limit (lib/core/test.py:806-883) per item: rows
 *       [d_offsets[b], d_offsets[b+1]) of d_scores [R,nc] / d_boxes [R,6nc] / d_keep_idx [R] (may be NULL) ->
 *       d_cls_boxes [batch,nc,max_rows,7], d_cls_keep [batch,nc,max_rows] (may be NULL), d_counts [batch,nc].
 *       Contract: d_offsets is non-decreasing and no item holds more than max_rows_per_item rows (the outputs and the
 *       scratch are sized for that many); rows of an item beyond max_rows_per_item are ignored.
 *   m3d_nms3d_batched                 nms_3d / nms_3d_volume (lib/utils/cython_nms_3d.pyx:39-159) per item of d_dets
 *       (item b at d_dets + b*item_stride_floats, count d_counts[b*count_stride] or max_boxes if d_counts is NULL):
 *       d_keep [batch,max_boxes] kept indices (ascending), d_num_keep [batch], and/or d_packed [batch,out_cap+1,7] = the
 *       kept rows, zero padded, with the count in element [out_cap][0] - the block m3d.shard all-gathers
 *       (lib/core/test.py:150-160). */
int m3d_fused_max_boxes(void);
/* Rows [0, min(d_counts[b], max_rows)) of every item b of d_src (item b at d_src + b*item_stride_bytes, rows of row_bytes, a multiple
 * of 4) packed back to back in item order into d_dst; d_offsets (may be NULL) receives the batch+1 row offsets.  The batched form of
 * `rois[:num]` per tile (lib/core/test.py:106-114 hands each tile's valid RoIs to the box head): no host round trip. */
int m3d_compact_rows(const void* d_src, size_t item_stride_bytes, size_t row_bytes, const int32_t* d_counts, int batch, int max_rows,
                     void* d_dst, int32_t* d_offsets, void* stream);
/* m3d_compact_rows for TWO row sets that share the counts (the RoIs and their score indices), one launch; h_counts (optional): a
 * device-accessible HOST mirror (pinned memory) of the clamped counts, written by the kernel - the caller waits for one stream event
 * instead of issuing a device-to-host copy. */
int m3d_compact_rows2(const void* d_src_a, size_t item_stride_bytes_a, size_t row_bytes_a, const void* d_src_b, size_t item_stride_bytes_b,
                      size_t row_bytes_b, const int32_t* d_counts, int batch, int max_rows, void* d_dst_a, void* d_dst_b,
                      int32_t* d_offsets, int32_t* h_counts, void* stream);
/* The box head's outputs in one launch (lib/modeling/fast_rcnn_heads.py:42-45, lib/core/test.py:225,250-251): d_outs [num_rois,
 * nc + 6 nc] = the cls_score and bbox_pred linears computed as ONE GEMM; d_rois [num_rois, 7] (batch, x1, y1, z1, x2, y2, z2) ->
 * d_cls [num_rois, nc] = softmax of the scores, d_bbox [num_rois, 6 nc] = the raw deltas, d_pred [num_rois, 6 nc] =
 * bbox_transform_3d(rois[:, 1:7], deltas, weights) clipped to (clip_slices, clip_height, clip_width) when clip_slices > 0. */
int m3d_box_head_outputs(const float* d_outs, const float* d_rois, int num_rois, int num_classes, const double* weights, double xform_clip,
                         double clip_slices, double clip_height, double clip_width, float* d_cls, float* d_bbox, float* d_pred, void* stream);
/* The whole detection box head as ONE call: RoIAlign3D (roi_res^3 bins) -> fc1 -> fc2 (f16x2 split, ReLU) -> cls_score | bbox_pred as one
 * GEMM -> m3d_box_head_outputs, launched on one stream exactly as m3d_roi_align3d_forward_ws, m3d_linear_f16x2_forward_bounds (twice),
 * m3d_linear_forward and m3d_box_head_outputs launch them (same plans, same kernels: bit-identical results).  It exists for the host
 * time between those launches: it follows the host read that sizes them, while the GPU is idle.  Every buffer is the caller's.
 *   fixed per network: fc1_packed / fc2_packed (m3d_linear_f16x2_pack of [fc1_out, channels * roi_res^3] and [fc2_out, fc1_out]), the
 *     biases, outs_weight [7 * num_classes, fc2_out] (cls_score rows, then bbox_pred rows) + outs_bias, the box-decoding weights;
 *   per call: features [batch, channels, slices, height, width], rois [num_rois, 7], clip (slices, height, width; clip[0] <= 0: none);
 *     feat_bound: feat_bound_slots floats whose largest is >= max |features| (what the last m3d_conv3d_zw_forward left), or NULL: fc1
 *     sweeps its input; fc1_bound: m3d_conv3d_zw_slots() floats, ZERO on entry, through which fc1 hands fc2 its operand bound, or
 *     NULL: fc2 sweeps its input;
 *   buffers: x [num_rois, channels * roi_res^3], h1 [num_rois, fc1_out], h2 [num_rois, fc2_out], outs [num_rois, 7 * num_classes]
 *     (intermediates), cls [num_rois, nc], bbox / pred [num_rois, 6 nc] (results), ws (m3d_box_head_workspace_bytes, 16-byte aligned).
 * num_rois <= 32 is M3D_EUNSUPPORTED (such a batch runs the fp32-input GEMM through the per-layer entries); 0 rows: nothing to do. */
typedef struct {
  const void* fc1_packed; const float* fc1_bias; const void* fc2_packed; const float* fc2_bias;
  const float* outs_weight; const float* outs_bias;
  int channels, roi_res, sampling_ratio, fc1_out, fc2_out, num_classes;
  float spatial_scale;
  double weights[6]; double xform_clip;
  const float* features; int batch, slices, height, width;
  const float* rois; int num_rois;
  double clip[3];
  const float* feat_bound; int feat_bound_slots; float* fc1_bound;
  float *x, *h1, *h2, *outs, *cls, *bbox, *pred;
  void* ws; size_t ws_bytes;
} m3d_box_head;
/* bytes of ws that serve every num_rois in 1 .. max_rois (0: a description the call does not take) */
size_t m3d_box_head_workspace_bytes(const m3d_box_head* head, int max_rois);
int m3d_box_head_forward(const m3d_box_head* head, void* stream);
size_t m3d_generate_proposals3d_batched_workspace_bytes(int batch, int A, int S, int H, int W, int pre_nms_topN);
/* m3d_generate_proposals3d_batched: out_rows = rows of the per-item output blocks, >= min(K, post_nms_topN) with NMS; with nms_thresh <= 0
 * every valid box of the K pre-NMS candidates is a proposal (generate_proposals_3d.py:167-171), so out_rows must be >= K - M3D_EINVAL
 * otherwise, never a silently truncated list. */
int m3d_generate_proposals3d_batched(const float* d_scores, const float* d_deltas, int batch, int A, int S, int H, int W,
                                     const double* anchors, double feat_stride, const double* im_info, int pre_nms_topN,
                                     int post_nms_topN, float nms_thresh, double min_size, double xform_clip,
                                     int first_batch_index, int out_rows, float* d_rois, float* d_probs,
                                     int64_t* d_keep_idx, int32_t* d_num, void* d_ws, size_t ws_bytes, void* stream);
size_t m3d_box_results3d_batched_workspace_bytes(int batch);
int m3d_box_results3d_batched(const float* d_scores, const float* d_boxes, const int64_t* d_keep_idx,
                              const int32_t* d_offsets, int batch, int num_classes, float score_thresh, float nms_thresh,
                              int detections_per_im, int max_rows_per_item, float* d_cls_boxes, int64_t* d_cls_keep,
                              int32_t* d_counts, void* d_ws, size_t ws_bytes, void* stream);
size_t m3d_nms3d_batched_workspace_bytes(int batch);
int m3d_nms3d_batched(const float* d_dets, size_t item_stride_floats, const int32_t* d_counts, int count_stride, int batch,
                      int max_boxes, float thresh, int by_volume, int out_cap, float* d_packed, int64_t* d_keep,
                      int32_t* d_num_keep, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Fully-connected layer: d_out [M,N] = act(d_x [M,K] . d_weight [N,K]^T + d_bias [N]).  Replaces the cuBLAS SGEMMs of
 * nn.Linear at lib/modeling/fast_rcnn_heads.py:84-85,114-115 (fc1: K = C*7^3 = 87 808, N = MLP_HEAD_DIM; fc2) and
 * :15-19,42-45 (cls_score, bbox_pred).  Operands keep PyTorch's layouts (both K-contiguous).  fp32 MFMA split-K GEMM;
 * partial sums live in d_ws (m3d_linear_workspace_bytes) and are reduced in a fixed order (deterministic).
 * K must be a multiple of 4 and both operands 16-byte aligned (else M3D_EUNSUPPORTED); d_bias may be NULL; relu != 0
 * fuses max(.,0). */
size_t m3d_linear_workspace_bytes(int M, int N, int K);
int m3d_linear_forward(const float* d_x, const float* d_weight, const float* d_bias, float* d_out, int M, int N, int K,
                       int relu, void* d_ws, size_t ws_bytes, void* stream);

/* The same layer on the bf16 matrix cores at fp32 accuracy ("bf16x3 split"): every fp32 operand is cut EXACTLY into three bf16
 * numbers (x = xh + xm + xl, 8 significand bits each) and six bf16 MFMAs (the products down to 2^-23 of the full product)
 * accumulate in fp32 what one fp32 MFMA step does - 16 / 6 of the fp32 matrix rate, error vs fp64 as the fp32 kernel's.
 * Finite operands only: an inf or NaN operand makes its output row / column NaN (fp32 would keep inf * finite = inf).
 * The weight is cut once: m3d_linear_bf16x3_pack writes three bf16 planes in tile order (m3d_linear_bf16x3_packed_bytes =
 * 6 bytes per weight, N rounded up to 128); x stays fp32 and is cut inside the kernel.  K must be a multiple of 32
 * (else M3D_EUNSUPPORTED / packed_bytes 0: use m3d_linear_forward).  Same split-K / fixed-order reduction contract. */
size_t m3d_linear_bf16x3_packed_bytes(int N, int K);
int m3d_linear_bf16x3_pack(const float* d_weight, int N, int K, void* d_packed, void* stream);
size_t m3d_linear_bf16x3_workspace_bytes(int M, int N, int K);
int m3d_linear_bf16x3_forward(const float* d_x, const void* d_packed, const float* d_bias, float* d_out, int M, int N, int K,
                              int relu, void* d_ws, size_t ws_bytes, void* stream);
/* The variant for many rows: 256 x 256 tiles, BOTH operands fp32 in HBM (d_weight = the nn.Linear weight itself, [N, K]) and cut on
 * the way to LDS - 16 KB of loads per 128 x 128 x 32 of work instead of 28-40, which is what bounds the bf16x3 GEMM.  Same accuracy
 * and contract as above; its own workspace size. */
size_t m3d_linear_bf16x3_w32_workspace_bytes(int M, int N, int K);
int m3d_linear_bf16x3_w32_forward(const float* d_x, const float* d_weight, const float* d_bias, float* d_out, int M, int N, int K,
                                  int relu, void* d_ws, size_t ws_bytes, void* stream);

/* Round 6 - the same layer with THREE products per fp32 product ("f16x2 split"; replaces the same cuBLAS SGEMMs,
 * lib/modeling/fast_rcnn_heads.py:84-85,114-115): each operand is scaled by a power of two (its largest magnitude just under 2^15) and
 * cut into two fp16 numbers, x s = xh + xl with |x s - xh - xl| <= 2^-22 |x s| (11 + 11 significand bits, round to nearest); three
 * v_mfma_f32_32x32x16_f16 products (hh, hl, lh) accumulate in fp32, the scales are undone exactly in the epilogue.  Dropped:
 * xl.wl and the cut residuals, each <= 2^-22 of the product and of random sign - below what the fp32 accumulation of K products
 * rounds in this kernel and in an SGEMM alike; tests compare both with fp64 on the shipped shape.  Half the matrix-core time of
 * m3d_linear_bf16x3_forward, 4 bytes per packed weight (packed_bytes also holds the weight's largest magnitude).
 * d_x_bound: device pointer to ONE float >= max|x| (m3d_absmax of x or of whatever bounds x: a RoIAlign output is a convex
 * combination of its feature map's values, so the map's largest magnitude does), or NULL: the call sweeps x itself first.
 * A bound smaller than max|x| overflows fp16 (inf / NaN outputs); a bound up to 2^8 too large costs no accuracy.  Finite operands only.
 * Workspace m3d_linear_f16x2_workspace_bytes (always >= 256, 16-byte aligned).  K % 32 == 0 else M3D_EUNSUPPORTED. */
int m3d_absmax(const float* d_x, long long n, float* d_out, void* stream);
size_t m3d_linear_f16x2_packed_bytes(int N, int K);
int m3d_linear_f16x2_pack(const float* d_weight, int N, int K, void* d_packed, void* stream);
size_t m3d_linear_f16x2_workspace_bytes(int M, int N, int K);
int m3d_linear_f16x2_forward(const float* d_x, const void* d_packed, const float* d_bias, float* d_out, int M, int N, int K,
                             int relu, const float* d_x_bound, void* d_ws, size_t ws_bytes, void* stream);
/* The same call with the bounds travelling as slot arrays, so that neither operand is swept: d_x_bound holds x_bound_slots floats whose
 * LARGEST is the bound (1: an m3d_absmax result; m3d_conv3d_zw_slots(): what m3d_conv3d_zw_forward left in d_out_max, or what this call
 * left in d_out_bound).  d_out_bound (or NULL): m3d_conv3d_zw_slots() floats, ZERO on entry, that receive max |d_out| from the launch
 * that stores d_out (the split-K reduce, or the GEMM's epilogue when K is not split), one atomic maximum per workgroup. */
int m3d_linear_f16x2_forward_bounds(const float* d_x, const void* d_packed, const float* d_bias, float* d_out, int M, int N, int K,
                                    int relu, const float* d_x_bound, int x_bound_slots, float* d_out_bound, void* d_ws, size_t ws_bytes,
                                    void* stream);

/* What the forward linear entry points launch for a shape (host only: nothing is launched, no device is touched).  kind 0:
 * m3d_linear_forward, 1: m3d_linear_bf16x3_forward, 2: m3d_linear_bf16x3_w32_forward, 3: m3d_linear_f16x2_forward(_bounds).  The answer
 * comes from the function the launch and its workspace query plan with, under the library's current options (tuning build: tune_fc_slices,
 * tune_fc_slices_tail, tune_fc_x3_rows): tile_rows x tile_cols = the workgroup tile, which names the kernel instantiation (kind 0: 128 x
 * 128; kinds 1 and 3: 128 x 128 or 256 x 128 on the packed planes; kinds 2 and 3: 256 x 256), slices = the K slices of every full row
 * tile, and for kind 0 slices_tail = those of the ragged last row tile (one or two 32-row blocks, run by the kernel's tail path; 1 where
 * there is none) and full_row_tiles = the row tiles in front of it; the other kinds have no tail path: slices_tail = slices and
 * full_row_tiles = all row tiles.  Any output pointer may be NULL.  M, N, K < 1 or an unknown kind: M3D_EINVAL; K % 4 != 0 (kind 0) or
 * K % 32 != 0 (the others): M3D_EUNSUPPORTED, as the launches. */
int m3d_linear_plan(int kind, int M, int N, int K, int* tile_rows, int* tile_cols, int* slices, int* slices_tail, int* full_row_tiles);

/* f-1 A/B: the fc1 GEMM with the RoIAlign gather in its A-operand loader - the [M, C * 343] RoIAlign output is never
 * written.  m3d_roi_align3d_tap_tables: the RoIs' per-axis sample tables (7^3 bins, sampling grid 2 - the shipped geometry) -> d_tab
 * (16 bytes x 3 axes x 14 samples per RoI) and d_roi_batch [num_rois]; m3d_linear_bf16x3_roi_forward: out[M, N] = act(RoIAlign3D(features,
 * rois) W^T + b) with d_packed = m3d_linear_bf16x3_pack(W) and K = channels * 343.  Same samples and weights as m3d_roi_align3d_forward
 * (another summation order).  Measured against the two-launch path (RoIAlign, then m3d_linear_bf16x3_forward) in profiles/r04_f1_ab.json:
 * the two-launch path is the product path. */
int m3d_roi_align3d_tap_tables(const float* d_rois, int num_rois, float spatial_scale, int batch, int slices, int height, int width,
                               void* d_tab, int32_t* d_batch, void* stream);
size_t m3d_linear_bf16x3_roi_workspace_bytes(int M, int N, int K);
int m3d_linear_bf16x3_roi_forward(const float* d_features, int batch, int channels, int slices, int height, int width, const void* d_tab,
                                  const int32_t* d_roi_batch, const void* d_packed, const float* d_bias, float* d_out, int M, int N, int relu,
                                  void* d_ws, size_t ws_bytes, void* stream);

/* Paste of the mask branch's soft masks into full-volume uint8 masks: segm_results, lib/core/test.py:886-945.
 * d_masks [num_dets, channels, M, M, M] (M = resolution, MRCNN.RESOLUTION); d_channel [num_dets]: the channel of each detection
 * (its class when MRCNN.CLS_SPECIFIC_MASK, else 0); d_boxes [num_dets, 6] = expand_boxes(ref_boxes, (M+2)/M).astype(int32) as
 * x0, y0, z0, x1, y1, z1 (inclusive; may leave the volume).  The (M+2)^3 zero-padded block of a detection is resized to its box's
 * (s, h, w) as skimage.transform.resize(order=1, mode='reflect', anti_aliasing=True) does (Gaussian pre-filter + order-1
 * map_coordinates, 'mirror' boundary; restated on scipy.ndimage's arithmetic, see csrc/mask_paste.hip), thresholded (> thresh) and
 * written into d_out [num_dets, depth, height, width] (uint8, zeroed here).  The Gaussian taps are the caller's: d_radius
 * [num_dets, 3] (z, y, x; 0 = axis not filtered) and d_weights [num_dets, 3, weight_stride] doubles, [d] = weight at distance d. */
size_t m3d_mask_paste3d_workspace_bytes(int num_dets, int resolution);
int m3d_mask_paste3d(const float* d_masks, int num_dets, int channels, int resolution, const int32_t* d_channel,
                     const int32_t* d_boxes, const int32_t* d_radius, const double* d_weights, int weight_stride, float thresh,
                     int depth, int height, int width, unsigned char* d_out, void* d_ws, size_t ws_bytes, void* stream);

/* norm1 pre-processing of a raw volume on the device: mask = im > 0; out = (im - mean(im[mask])) / std(im[mask])
 * (np.std: population).  Replaces the host NumPy code of lib/utils/blob.py:179-184 (float32; f32_arith = 1) and
 * tools/infer_simple.py:180-183 (float64, crops cast to float32 at :217; f32_arith = 0), so the raw uint16 volume is what
 * crosses PCIe.  in_dtype: 0 = uint16, 1 = float32.  Statistics are two-pass fp64 sums in a fixed order (deterministic);
 * d_stats (optional, 3 doubles) receives mean, std, count. */
size_t m3d_norm1_workspace_bytes(void);
int m3d_norm1(const void* d_in, int in_dtype, int64_t n, int f32_arith, float* d_out, double* d_stats, void* d_ws,
              size_t ws_bytes, void* stream);
/* batch volumes of n voxels each, contiguous; each with its own statistics (one launch per pass for the whole batch).
 * d_stats [batch,3] or null; d_ws: batch * m3d_norm1_workspace_bytes() */
int m3d_norm1_batched(const void* d_in, int in_dtype, int batch, int64_t n, int f32_arith, float* d_out, double* d_stats, void* d_ws,
                      size_t ws_bytes, void* stream);
/* The statistics alone: the same two passes and a finish that writes mean, std, count to d_stats [batch,3] (required); no normalised
 * volume is written.  The same partials summed in the same order: the same bits as d_stats of m3d_norm1 / m3d_norm1_batched.
 * d_ws: batch * m3d_norm1_workspace_bytes(). */
int m3d_norm1_stats(const void* d_in, int in_dtype, int batch, int64_t n, double* d_stats, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Peak-response back-propagation on cropped windows (all kept peaks of a tile as one batch).  Replaces the
 * per-detection `class_response_maps.backward(...)` loop of lib/prm/peak_response_mapping_3d.py:157-172 and
 * the hooks of lib/prm/peak_backprop_3d.py:8-34.  Windows are cubes in virtual coordinates (positions
 * outside the tile are zero), d_origin* are int32 [num_peaks,3] = (z,y,x).
 *   m3d_prm_seed      sigmoid' + the 1x1x1 RPN_cls_score conv for one-hot seeds: d_peaks int32 [P,4] =
 *                     (anchor,s,h,w); d_prob/d_norm_cls [A,S,H,W]; d_w_cls [A,C]; d_h [C,S,H,W] (the ReLU'd
 *                     RPN_conv output) and its min; writes d_out [P,C] (a 1^3 window per peak at (s,h,w)).
 *   m3d_prm_prepare   upper window d_gup [P,C,U,U,U] (gradient w.r.t. this layer's post-activation output, at
 *                     d_origin_up) -> this layer's conv-input window d_out [P,C,Wn,Wn,Wn], Wn = (pool?2:1)*U +
 *                     2*border: max-unpool routing by d_argmax (if pool), ReLU mask (d_xnext > 0; pooled values
 *                     if pool), * d_scale[c] (BatchNorm, may be NULL), / (|norm|+1e-10) with norm < 1e-10 -> 0.
 *   m3d_prm_stem_prepare_weights  d_weight [C,1,5,5,5] -> d_wf [C,125] = flipped relu(W) (once per model).
 *   m3d_prm_stem_dgrad backward-data of conv1a (5^3, one output channel) with d_wf, times (data - offset),
 *                     clamp(min=0); d_out [P,Wn^3]; d_sums [P] = per-peak sum (for prm / prm.sum()).
 *   m3d_prm_scatter   dense [P,D,H,W] = window / sum at each peak's origin, 0 / sum elsewhere (every voxel is written: a peak whose
 *                     map sums to 0 - saturated sigmoid - gives NaN everywhere, as the reference's prm / prm.sum() does).
 * ------------------------------------------------------------------------------------------------------- */
int m3d_prm_seed(const int32_t* d_peaks, int num_peaks, const float* d_prob, const float* d_norm_cls,
                 const float* d_w_cls, const float* d_h, const float* d_h_offset, int A, int C, int S, int H, int W,
                 float* d_out, void* stream);
/* the same + d_origin_out int32 [P,3] (or null): every peak's (s, h, w), the origin of its 1^3 window */
int m3d_prm_seed_ex(const int32_t* d_peaks, int num_peaks, const float* d_prob, const float* d_norm_cls,
                    const float* d_w_cls, const float* d_h, const float* d_h_offset, int A, int C, int S, int H, int W,
                    float* d_out, int32_t* d_origin_out, void* stream);
/* Peak selection on the device (lib/prm/peak_response_mapping_3d.py:124-139,161-163): class 1's kept detections d_dets [rows,7]
 * (x1,y1,z1,x2,y2,z2,score; the first *d_count rows are valid) with their flat score indices d_keep_idx into (S,H,W,A)
 * (generate_proposals_3d.py:160) -> the detections whose score > peak_threshold, in order: *d_num (<= cap), d_peaks int32 [cap,4] =
 * (anchor,s,h,w) = unravel_index(idx,(S,H,W,A)) reordered, d_out_dets [cap,7].  h_num / h_peaks / h_out_dets (optional, may be NULL):
 * device-accessible HOST mirrors (pinned memory) the kernel writes as well, so that the caller learns count, peaks and detections
 * from one stream event instead of three read-backs.  One workgroup; no host synchronisation. */
int m3d_prm_select_peaks(const float* d_dets, const int64_t* d_keep_idx, const int32_t* d_count, int rows, float peak_threshold,
                         int A, int S, int H, int W, int cap, int32_t* d_num, int32_t* d_peaks, float* d_out_dets, int32_t* h_num,
                         int32_t* h_peaks, float* h_out_dets, void* stream);
/* the same + d_prob [A,S,H,W] (the class response map, may be null) -> d_dead / h_dead int32 [cap] (each may be null): 1 for a peak whose
 * sigmoid derivative (1 - y) y is exactly 0 - its back-propagated map is all zero (`prm / prm.sum()` = 0 / 0) and need not be computed */
int m3d_prm_select_peaks_ex(const float* d_dets, const int64_t* d_keep_idx, const int32_t* d_count, int rows, float peak_threshold,
                            int A, int S, int H, int W, int cap, int32_t* d_num, int32_t* d_peaks, float* d_out_dets, int32_t* h_num,
                            int32_t* h_peaks, float* h_out_dets, const float* d_prob, int32_t* d_dead, int32_t* h_dead, void* stream);
/* Geometry of the strip layouts [C, n, n, L] of a window batch (all peaks side by side along x; see m3d_prm_prepare_ex): mode 1 =
 * pitch n + 1 for the exactly-local F(2x2,3x3) kernel, mode 2 = quad-aligned windows for the F(2x4,3x3) kernel (no output quad of one
 * window reads another window's columns).  Returns L; window p occupies columns lead + p * pitch .. + n - 1, all others are zero. */
int64_t m3d_prm_strip_geometry(int window, int mode, int num_peaks, int32_t* pitch, int32_t* lead);
int m3d_prm_prepare(const float* d_gup, const int32_t* d_origin_up, int num_peaks, int channels, int up_size, int pool,
                    int border, const uint8_t* d_argmax, const float* d_xnext, int up_depth, int up_height,
                    int up_width, const float* d_scale, const float* d_norm, int depth, int height, int width,
                    float* d_out, int32_t* d_origin_out, void* stream);
int m3d_prm_stem_prepare_weights(const float* d_weight, int channels, float* d_wf, void* stream);
int m3d_prm_stem_dgrad(const float* d_gn, const float* d_wf, const float* d_data, const float* d_data_offset,
                       const int32_t* d_origins, int num_peaks, int channels, int win, int depth, int height,
                       int width, float* d_out, float* d_sums, void* stream);
int m3d_prm_scatter(const float* d_windows, const float* d_sums, const int32_t* d_origins, int num_peaks, int win,
                    int depth, int height, int width, float* d_dense, void* stream);

/* Round 2: the stem step of the peak back-propagation on the matrix cores, with the prepare step fused (replaces
 * m3d_prm_prepare(pool = 1, border = 2) + m3d_prm_stem_dgrad for 32 stem channels and even window sizes; same results up to
 * fp32 summation order).
 *   m3d_prm_den_pool   peak-independent denominator map of a conv + MaxPool3d(2,2) layer, once per tile: d_den [C,UD,UH,UW] =
 *                      |N| + 1e-10 at the argmax child where the pooled activation is > 0 and N >= 1e-10, else 0
 *                      (lib/prm/peak_backprop_3d.py:30-33 with the ReLU mask and the max-unpool routing folded in).
 *   m3d_prm_stem_mfma_prepare_weights  conv1a weight [32,1,5,5,5] -> d_wa [80,64]: tap-flipped relu(W) in MFMA A-operand order.
 *   m3d_prm_stem_dgrad_fused_supported 1 when the fused kernel has a configuration for (channels, up_size).
 *   m3d_prm_stem_dgrad_fused  d_gup [P,32,U,U,U] (gradient w.r.t. the pooled stem output), d_origin_up int32 [P,3] (pooled
 *                      coordinates) -> d_out [P,Wn,Wn,Wn] (Wn = 2U + 4) = clamp((data - offset) * dgrad, min 0), d_sums [P],
 *                      d_origins_out int32 [P,3] = 2 * origin_up - 2   (peak_response_mapping_3d.py:169-171). */
int m3d_prm_den_pool(const uint8_t* d_argmax, const float* d_xnext, const float* d_norm, int channels, int up_depth, int up_height,
                     int up_width, int depth, int height, int width, float* d_den, void* stream);
int m3d_prm_stem_mfma_prepare_weights(const float* d_weight, int channels, float* d_wa, void* stream);
int m3d_prm_stem_dgrad_fused_supported(int channels, int up_size);
int m3d_prm_stem_dgrad_fused(const float* d_gup, const int32_t* d_origin_up, int num_peaks, int channels, int up_size,
                             const float* d_den, const uint8_t* d_argmax, const float* d_scale, int up_depth, int up_height,
                             int up_width, const float* d_wa, const float* d_data, const float* d_data_offset, int depth, int height,
                             int width, float* d_out, float* d_sums, int32_t* d_origins_out, void* stream);

/* Strip layout for window batches: the P windows of n^3 voxels side by side along x, one separator column after each -
 * [C, n, n, P*(n+1)] instead of [P, C, n, n, n] - so that m3d_conv3d_wino2_forward convolves the whole batch as ONE wide volume
 * (its 64-wide tiles fit 38 / 40-voxel windows badly, a 2 600-voxel strip well).  That kernel has no PreHook epilogue, so the
 * consumer of its output applies the multiply by (X - offset) of peak_backprop_3d.py:16-18:
 *   m3d_prm_prepare_ex           m3d_prm_prepare with in_strip / out_strip (0 batch-major, 1 strip) and d_up_offset (non-null: d_gup
 *                                is a bare backward-data result, multiplied here by (d_xnext - *d_up_offset)); writes the zero separators.
 *   m3d_prm_stem_dgrad_fused_ex  m3d_prm_stem_dgrad_fused with gup_strip and (d_xnext [32,UD,UH,UW], d_up_offset) for the same purpose. */
int m3d_prm_prepare_ex(const float* d_gup, const int32_t* d_origin_up, int num_peaks, int channels, int up_size, int pool, int border,
                       const uint8_t* d_argmax, const float* d_xnext, int up_depth, int up_height, int up_width, const float* d_scale,
                       const float* d_norm, int depth, int height, int width, int in_strip, int out_strip, const float* d_up_offset,
                       float* d_out, int32_t* d_origin_out, void* stream);
int m3d_prm_stem_dgrad_fused_ex(const float* d_gup, int gup_strip, const float* d_xnext, const float* d_up_offset,
                                const int32_t* d_origin_up, int num_peaks, int channels, int up_size, const float* d_den,
                                const uint8_t* d_argmax, const float* d_scale, int up_depth, int up_height, int up_width,
                                const float* d_wa, const float* d_data, const float* d_data_offset, int depth, int height, int width,
                                float* d_out, float* d_sums, int32_t* d_origins_out, void* stream);
/* Depth-clipped ("slab") strips, round 4: [C, zn, n, L] with zn = the depth of the LAYER's map - plane k of every window is plane k
 * of the map - instead of the n planes of each window.  Where a tile is thinner than the receptive-field cone (the nuclei tile's
 * stride-2 maps: 32 planes against windows of 38 / 40) the planes of a window outside the volume carry zero gradient in and are never
 * read out (peak_backprop_3d.py:30-33 only ever divides inside the map); a slab strip does not store, convolve or stream them.  y / x
 * geometry, separators and origins are those of the window strips (origins stay the cone's, z possibly negative).
 *   in_slab / out_slab / gup_slab != 0: that strip is a slab strip (d_gup: up_depth planes; d_out: depth planes); strip layouts only. */
int m3d_prm_prepare_ex2(const float* d_gup, const int32_t* d_origin_up, int num_peaks, int channels, int up_size, int pool, int border,
                        const uint8_t* d_argmax, const float* d_xnext, int up_depth, int up_height, int up_width, const float* d_scale,
                        const float* d_norm, int depth, int height, int width, int in_strip, int in_slab, int out_strip, int out_slab,
                        const float* d_up_offset, float* d_out, int32_t* d_origin_out, void* stream);
/* ... and d_peak_max [num_peaks x 32] (or NULL: exactly the call above): element 32 p = the largest |value| written for peak p (zeroed and
 * filled by this call; one cache line per peak) - the per-window operand bound m3d_conv3d_zw_forward_strip takes, so that the strip is never swept for it. */
int m3d_prm_prepare_ex3(const float* d_gup, const int32_t* d_origin_up, int num_peaks, int channels, int up_size, int pool,
                        int border, const uint8_t* d_argmax, const float* d_xnext, int up_depth, int up_height, int up_width,
                        const float* d_scale, const float* d_norm, int depth, int height, int width, int in_strip, int in_slab,
                        int out_strip, int out_slab, const float* d_up_offset, float* d_out, int32_t* d_origin_out,
                        float* d_peak_max, void* stream);
int m3d_prm_stem_dgrad_fused_ex2(const float* d_gup, int gup_strip, int gup_slab, const float* d_xnext, const float* d_up_offset,
                                 const int32_t* d_origin_up, int num_peaks, int channels, int up_size, const float* d_den,
                                 const uint8_t* d_argmax, const float* d_scale, int up_depth, int up_height, int up_width,
                                 const float* d_wa, const float* d_data, const float* d_data_offset, int depth, int height, int width,
                                 float* d_out, float* d_sums, int32_t* d_origins_out, void* stream);
/* Which kernel a shape runs (host only, no GPU touched; the launchers ask the same functions, so a test can name the path it checks):
 *   m3d_prm_prepare_plan     the kernel of m3d_prm_prepare_ex3 for a 16-byte-aligned d_out: 0 element (one thread per voxel), 1 / 2 / 3
 *                            quad (four columns per thread on the quad-aligned strip, 8 / 16 / 32 lanes across a row), 4 pool (one
 *                            thread per 2x2x2 block); or the negative M3D_E* code the call returns for this shape.  `depth` (> 0) decides
 *                            with out_slab only.  An unaligned d_out runs the element kernel in place of a quad one.
 *   m3d_prm_stem_dgrad_plan  the thread layout of m3d_prm_stem_dgrad for win^3 windows: 0 = 32 x 16 x 8 voxels per workgroup,
 *                            1 = 40 x 12 x 8; M3D_EINVAL for win <= 0. */
int m3d_prm_prepare_plan(int channels, int num_peaks, int up_size, int pool, int border, int out_strip, int out_slab, int depth);
int m3d_prm_stem_dgrad_plan(int win);

/* 3x3x3 "same" convolution at fp32 accuracy on the bf16 matrix cores (csrc/conv3d_x3.hip; round 4): out = conv3d(x - *d_in_offset, W',
 * padding = 1) with W' = W or relu(W) chosen at pack time - the norm convolution of lib/prm/peak_backprop_3d.py:37-44 (pr_conv3d's second
 * F.conv3d: N = conv(X - min X, relu(W))), which has to stay an exact sum of products.  Both fp32 operands are cut into three bf16 pieces
 * (exact), six bf16 MFMA products per fp32 product: the error is the fp32 kernel's, non-negative operands give exact zeros exactly where
 * the fp32 sum has them.  cin must be a multiple of 16 (m3d_conv3d_x3_supported); zero padding applies to the SHIFTED input.
 *   m3d_conv3d_x3_packed_bytes / _pack   weight [cout, cin, 3, 3, 3] fp32 -> packed pieces (once per model; relu_weights: relu(W))
 *   m3d_conv3d_x3_forward                 x [B, cin, D, H, W] -> out [B, cout, D, H, W]; d_in_offset: device scalar or null */
size_t m3d_conv3d_x3_packed_bytes(int cin, int cout);
int m3d_conv3d_x3_supported(int cin, int cout);
int m3d_conv3d_x3_pack(const float* d_weight, int cin, int cout, int relu_weights, void* d_packed, void* stream);
int m3d_conv3d_x3_forward(const float* d_x, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
                          int width, const float* d_in_offset, void* stream);
/* The same with a caller workspace (m3d_conv3d_x3_workspace_bytes; 0 = none needed): maps too small to fill the chip are cut along K into
 * up to four ranges of input channels, one workgroup each, whose partial sums a second kernel adds in range order (deterministic). */
size_t m3d_conv3d_x3_workspace_bytes(int batch, int cin, int cout, int depth, int height, int width);
int m3d_conv3d_x3_forward_ws(const float* d_x, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
                             int width, const float* d_in_offset, void* d_workspace, size_t workspace_bytes, void* stream);
/* Round 6 - the same convolution with the "f16x2 split" of m3d_linear_f16x2_forward: both operands scaled by a power of two and cut into
 * two fp16 numbers (22 bits), three v_mfma_f32_32x32x16_f16 products per fp32 product (replaces the same F.conv3d call,
 * lib/prm/peak_backprop_3d.py:37-44).  d_in_max: device pointer to max(x) when d_in_offset is given (the operand x - offset is bounded by
 * max - offset), to max |x| when it is not (m3d_reduce_minmax_multi / m3d_absmax).  For the norm convolutions every operand is >= 0 and
 * every PRODUCT TRIPLE hh + hl + lh is >= 0: a result is zero exactly when every x w is, as with the fp32 and bf16x3 kernels.  Pack with
 * m3d_conv3d_x3f_pack (4 bytes per weight + the weight's largest magnitude); workspace / launch units as m3d_conv3d_x3_*. */
size_t m3d_conv3d_x3f_packed_bytes(int cin, int cout);
int m3d_conv3d_x3f_pack(const float* d_weight, int cin, int cout, int relu_weights, void* d_packed, void* stream);
int m3d_conv3d_x3f_forward_ws(const float* d_x, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
                              int width, const float* d_in_offset, const float* d_in_max, void* d_workspace, size_t workspace_bytes,
                              void* stream);
/* Workgroups m3d_conv3d_x3_forward_ws launches for this shape when given its workspace (spatial x cout tiles, times the K ranges): the
 * library's own decision, for callers that choose between this kernel and m3d_conv3d_forward by how well a launch fills the chip. */
long long m3d_conv3d_x3_launch_units(int batch, int cin, int cout, int depth, int height, int width);

/* Round 6 - the FORWARD 3x3x3 convolution + eval-BN + ReLU [+ MaxPool3d(2,2)] of lib/modeling/DSN.py:57-68 (and rpn_heads.py:94-96) on the
 * f16 matrix cores at fp32 accuracy: the f16x2 split (three fp16 products per fp32 product) with Winograd F(2,3) along z (36 instead of 54
 * products per output pair): csrc/conv3d_zw.hip.  cin must be a multiple of 16; depth >= 2, height >= 4, width >= 12 (pool: even extents,
 * width >= 24) - m3d_conv3d_zw_supported.  d_in_max: device array of m3d_conv3d_zw_slots() (= 32) non-negative floats whose LARGEST is
 * >= max |d_in| (the operand scale; an input beyond the bound overflows fp16); d_out_max (or NULL): the same kind of array for d_out,
 * updated with atomic maxima - the caller zeroes it before the launch and hands it to the next layer as its d_in_max, so that a chain of
 * layers needs one sweep (m3d_conv3d_zw_bound_of) for its first input only.  relu / d_scale / d_shift as m3d_conv3d_forward; pool = 1:
 * d_out is [batch, cout, depth/2, height/2, width/2].  Differences to the fp32 kernels: ~1e-6 of the largest output. */
int m3d_conv3d_zw_supported(int cin, int cout, int depth, int height, int width, int pool);
size_t m3d_conv3d_zw_packed_bytes(int cin, int cout);
int m3d_conv3d_zw_pack(const float* d_weight, int cin, int cout, void* d_packed, void* stream);
/* The pack of the BACKWARD-DATA conv of a layer, straight from the layer's own parameter d_weight [cout, cin, 3, 3, 3] (the FORWARD
 * layout): taps flipped and channel roles swapped while packing, so the pack's input channels are `cout` and its output channels `cin`.
 * d_packed: m3d_conv3d_zw_packed_bytes(cout, cin) bytes, equal to m3d_conv3d_zw_pack of the flipped, transposed, contiguous copy
 * (w.flip(2, 3, 4).transpose(0, 1)) byte for byte, the largest magnitude behind the fragments included.  M3D_EINVAL, before any pointer
 * is followed: a NULL pointer, a non-positive count, cout % 16 != 0. */
int m3d_conv3d_zw_pack_dgrad(const float* d_weight, int cin, int cout, void* d_packed, void* stream);
int m3d_conv3d_zw_slots(void);
/* Workgroup units of an m3d_conv3d_zw_forward launch on this shape ((64 output channels) x (32 x 4 x 2 voxels, or 16 x 8 x 2 on maps
 * narrower than 24) per unit): the library's own tile choice, for callers that choose between this kernel and the fp32 ones by how well a
 * launch fills the chip (host only; says nothing about m3d_conv3d_zw_supported). */
long long m3d_conv3d_zw_launch_units(int batch, int cin, int cout, int depth, int height, int width);
int m3d_conv3d_zw_bound_of(const float* d_x, long long n, float* d_slots, void* stream);
int m3d_conv3d_zw_forward(const float* d_in, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
                          int width, const float* d_scale, const float* d_shift, int relu, int pool, const float* d_in_max,
                          float* d_out_max, void* stream);
/* The 3x3x3 convolution (stride 1, pad 1) [+ scale / shift + ReLU] on NARROW maps - width <= 8: the per-RoI convs on 7^3 RoI grids - on
 * the f16 matrix cores at fp32 accuracy: the f16x2 split in the DIRECT form (27 taps, no Winograd; a zero product stays exact), csrc/conv3d_zn.hip.
 * [batch, cin, depth, height, width] with cin % 16 == 0, width <= 8, any cout / depth / height / batch >= 1, cin * depth * height * width
 * < 2^29 (m3d_conv3d_zn_supported).  One workgroup per unit of (64 output channels) x (8 x 8 x 4 voxels), the whole K inside it: no
 * atomics on d_out, bit-identical run to run; every element of d_out is written.  d_in_max / d_out_max as m3d_conv3d_zw_forward's
 * (m3d_conv3d_zw_slots() floats; d_out_max zeroed by the caller, or NULL); out = acc x (1 / (s_a s_b)) [x d_scale[c]] + d_shift[c], then
 * ReLU.  m3d_conv3d_zn_pack_dgrad: the pack of the backward-data conv straight from the forward parameter [cout, cin, 3, 3, 3], equal to
 * m3d_conv3d_zn_pack of w.flip(2, 3, 4).transpose(0, 1) byte for byte, m3d_conv3d_zn_packed_bytes(cout, cin) bytes (cout % 16 == 0).
 * M3D_EINVAL (a NULL pointer, a non-positive count) and M3D_EUNSUPPORTED (a shape m3d_conv3d_zn_supported refuses) before any pointer is
 * followed. */
int m3d_conv3d_zn_supported(int cin, int cout, int depth, int height, int width);
size_t m3d_conv3d_zn_packed_bytes(int cin, int cout);
int m3d_conv3d_zn_pack(const float* d_weight, int cin, int cout, void* d_packed, void* stream);
int m3d_conv3d_zn_pack_dgrad(const float* d_weight, int cin, int cout, void* d_packed, void* stream);
long long m3d_conv3d_zn_launch_units(int batch, int cin, int cout, int depth, int height, int width);
int m3d_conv3d_zn_forward(const float* d_in, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth, int height,
                          int width, const float* d_scale, const float* d_shift, int relu, const float* d_in_max, float* d_out_max,
                          void* stream);
/* m3d_conv3d_zn_forward at dilation 1 or 2 with padding = dilation: dilation 2 / padding 2 is the 3x3x3 "same" convolution of the mask
 * head at MRCNN.DILATION = 2 (lib/modeling/mask_rcnn_heads.py:141-151, lib/core/config.py:767) on the per-RoI 7^3 grids.  The same
 * kernel instantiated for a 2-voxel halo (csrc/conv3d_zn.hip): the same unit of (64 output channels) x (8 x 8 x 4 voxels), the same
 * f16x2 cut, three MFMAs per product, fp32 accumulation, exact un-scale, epilogue and d_out_max; no atomics on d_out, bit-identical run
 * to run, every element of d_out written, a zero product exact.  The weight packs do not depend on the dilation: d_packed is an
 * m3d_conv3d_zn_pack pack for a forward conv.  With the m3d_conv3d_zn_pack_dgrad pack of a layer's weights, that layer's output
 * gradient as d_in, cin and cout exchanged, d_scale = d_shift = NULL and relu = 0 it is the layer's backward-data at the same dilation
 * (padding = dilation makes the transposed conv the same dilated conv of the flipped, transposed weights, as for
 * m3d_conv3d_forward_dilated).
 * m3d_conv3d_zn_dilated_supported: dilation 1 what m3d_conv3d_zn_supported says, dilation 2 the same limits, any other dilation 0.
 * m3d_conv3d_zn_dilated_launch_units: host only, the workgroups of such a launch (0 for a dilation that is not supported).
 * m3d_conv3d_zn_dilated_forward: dilation 1 IS m3d_conv3d_zn_forward (the same launch, the same bits).  Refusals, all before a pointer
 * is followed or anything is launched: M3D_EINVAL a NULL d_in / d_packed / d_out / d_in_max or batch <= 0; M3D_EUNSUPPORTED another
 * dilation, a shape m3d_conv3d_zn_dilated_supported refuses, 2^31 units or more. */
int m3d_conv3d_zn_dilated_supported(int cin, int cout, int depth, int height, int width, int dilation);
long long m3d_conv3d_zn_dilated_launch_units(int batch, int cin, int cout, int depth, int height, int width, int dilation);
int m3d_conv3d_zn_dilated_forward(const float* d_in, const void* d_packed, float* d_out, int batch, int cin, int cout, int depth,
                                  int height, int width, int dilation, const float* d_scale, const float* d_shift, int relu,
                                  const float* d_in_max, float* d_out_max, void* stream);
/* The convolution of m3d_conv3d_zw_forward on a PRM window strip [cin, depth, height, width] (peak_backprop_3d.py:8-34 batched over peaks: the windows of all
 * peaks side by side along x, cell p = columns [pitch p, pitch (p + 1)), pitch a multiple of 4 - m3d_prm_strip_geometry mode 2) with ONE
 * OPERAND SCALE PER WINDOW: d_col_bound [num_peaks x 32], element 32 p = the largest |input| of window p (one cache line per window;
 * m3d_prm_strip_absmax: one sweep, rows = cin x depth x height; or the d_peak_max of m3d_prm_prepare_ex3).  The gradients of different peaks differ by orders of magnitude: each keeps its own 22 bits, and a window's
 * outputs do not depend on which other windows share the strip.  F(2,3) along z and the direct (y, x) taps are exactly local: a window's
 * outputs read nothing beyond its own 3^3 supports.  No scale / shift / ReLU / pool; width >= 24. */
int m3d_prm_strip_absmax(const float* d_strip, long long rows, int L, int pitch, int num_peaks, float* d_out, void* stream);
int m3d_conv3d_zw_forward_strip(const float* d_in, const void* d_packed, float* d_out, int cin, int cout, int depth, int height,
                                int width, const float* d_col_bound, int num_peaks, int pitch, void* stream);
/* m3d_conv3d_zw_forward_strip FUSED with the prepare step of the layer below: the contract of m3d_prm_strip_dgrad_prepare (the fp32
 * F(2x4,3x3) kernel's fused form), the same arguments plus d_col_bound (and d_packed from m3d_conv3d_zw_pack).  The strip it writes is the
 * two launches' (m3d_conv3d_zw_forward_strip, then m3d_prm_prepare_ex2 with pool = 0, border = 1) bit for bit; the bare gradient strip is
 * never stored.  M3D_EUNSUPPORTED where the kernel has no configuration (the caller takes the two launches). */
int m3d_prm_strip_dgrad_prepare_zw(const float* d_gn, const void* d_packed, int cin, int cout, int num_peaks, int window, int in_slab,
                                   const int32_t* d_origin, const float* d_xnext, const float* d_norm, const float* d_scale,
                                   const float* d_up_offset, int depth, int height, int width, int out_slab,
                                   const float* d_col_bound, float* d_out, int32_t* d_origin_out, void* stream);

/* Round 5: backward-data of a 3^3 conv on the quad-aligned strip FUSED with the prepare step of the layer below (no pooling between them):
 * d_gn [cin, in_planes, window, L(window)] (m3d_prm_prepare_ex2's out_strip = 2 layout; in_slab: the map's planes), d_packed =
 * m3d_conv3d_wino2_pack_weights of the backward-data weights -> d_out [cout, out_planes, window + 2, L(window + 2)], the strip
 * m3d_prm_prepare_ex2(in_strip = 2, out_strip = 2, pool = 0, border = 1, d_up_offset) would have made of the conv's result, bit for bit;
 * d_origin_out = d_origin - 1.  d_out is zero-filled by the call.  M3D_EUNSUPPORTED: take the two-launch path. */
int m3d_prm_strip_dgrad_prepare(const float* d_gn, const float* d_packed, int cin, int cout, int num_peaks, int window, int in_slab,
                                const int32_t* d_origin, const float* d_xnext, const float* d_norm, const float* d_scale,
                                const float* d_up_offset, int depth, int height, int width, int out_slab, float* d_out,
                                int32_t* d_origin_out, void* stream);

/* Backward-data of a 3x3x3 conv with relu(W) on batches of SMALL windows (win in {3, 5, 7}: the stride-8 / 4 stages of the peak
 * back-propagation), peaks batched densely into the GEMM N dimension; same operation as m3d_conv3d_forward_windowed on
 * dgrad-packed weights: d_gn [P, cout_fwd, win^3] -> d_out [P, cin_fwd, win^3] = (d_full[co][origin + v] - *d_full_offset) *
 * sum relu(W)[ci][co][26 - t] * gn[p, ci][v + t - 1]  (lib/prm/peak_backprop_3d.py:16-18,41-42).  d_weight: the forward conv's
 * [cout_fwd, cin_fwd, 3, 3, 3]; pack once per model. */
size_t m3d_prm_small_dgrad_packed_bytes(int cout_fwd, int cin_fwd);
int m3d_prm_small_dgrad_pack(const float* d_weight, int cout_fwd, int cin_fwd, float* d_packed, void* stream);
int m3d_prm_small_dgrad(const float* d_gn, const float* d_packed, int num_peaks, int cout_fwd, int cin_fwd, int win,
                        const float* d_full, const float* d_full_offset, const int32_t* d_origins, int depth, int height, int width,
                        float* d_out, void* stream);
/* Round 6 - the same operation on the f16 matrix cores ("f16x2 split", see m3d_linear_f16x2_forward): both operands scaled by a power of
 * two and cut into two fp16 numbers (22 bits), three v_mfma_f32_32x32x16_f16 products per fp32 product.  The gradient windows are
 * scaled PER PEAK (every peak's [cout_fwd, win^3] block is swept once for its largest magnitude into the workspace; peaks differ by
 * orders of magnitude), relu(W) per layer at pack time.  A column's result depends on its own peak only: a sub-batch gives the batch's
 * rows bit for bit.  cout_fwd must be a multiple of 16 (m3d_prm_small_dgrad_f16_supported), win in {3, 5, 7}; workspace
 * m3d_prm_small_dgrad_f16_workspace_bytes(num_peaks).  Agreement with m3d_prm_small_dgrad: ~1e-6 of the layer's largest value. */
int m3d_prm_small_dgrad_f16_supported(int cout_fwd, int cin_fwd);
size_t m3d_prm_small_dgrad_f16_packed_bytes(int cout_fwd, int cin_fwd);
int m3d_prm_small_dgrad_f16_pack(const float* d_weight, int cout_fwd, int cin_fwd, void* d_packed, void* stream);
size_t m3d_prm_small_dgrad_f16_workspace_bytes(int num_peaks);
int m3d_prm_small_dgrad_f16(const float* d_gn, const void* d_packed, int num_peaks, int cout_fwd, int cin_fwd, int win,
                            const float* d_full, const float* d_full_offset, const int32_t* d_origins, int depth, int height, int width,
                            float* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* Backward-data of the 5^3 / Cin = 1 stem conv for autograd (what cuDNN dgrad computes for conv1a when the input requires
 * grad: the reference's PRM mode, lib/prm/peak_response_mapping_3d.py:88 + lib/prm/peak_backprop_3d.py:37-44, lib/modeling/DSN.py:19).
 *   m3d_conv3d_stem5_prepare_dgrad_weights  d_weight [C,1,5,5,5] -> d_wf [C,125], taps flipped (no ReLU: the caller passes
 *                                           whatever weight the conv ran with)
 *   m3d_conv3d_stem5_dgrad                  d_grad_out [batch,C,D,H,W] -> d_grad_in [batch,1,D,H,W] */
int m3d_conv3d_stem5_prepare_dgrad_weights(const float* d_weight, int channels, float* d_wf, void* stream);
int m3d_conv3d_stem5_dgrad(const float* d_grad_out, const float* d_wf, float* d_grad_in, int batch, int channels, int depth,
                           int height, int width, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * PRM post-processing feeding the Otsu step.
 *   m3d_prm_quantize_u8  per map: fm -= min; fm /= max; fm *= 255 -> uint8, float32 arithmetic
 *                        (tools/infer_simple.py:233-238; what the reference stores in its PRM TIFFs).
 *   m3d_roi_normalize    per detection: crop the inclusive box (x1,y1,z1,x2,y2,z2: int32 [R,6], tile coords) from
 *                        the uint16 tile and from the RoI's own uint8 PRM map, normalise both to similar ranges and
 *                        write them back to back at d_offsets[r] (int64 [R+1], offsets[r+1]-offsets[r] = crop voxels):
 *                        mode 0 = soma  (tools/binarization_soma.py:81-91), mode 1 = nuclei
 *                        (tools/binarization_nuclei.py:107-121).  float64 arithmetic, np.round / astype semantics.
 *                        The outputs are exactly the (image, prm) inputs of m3d_otsu2d_batch.
 * ------------------------------------------------------------------------------------------------------- */
int m3d_prm_quantize_u8(const float* d_prm, int num_maps, int64_t voxels_per_map, uint8_t* d_out, void* stream);
int m3d_roi_normalize(const uint16_t* d_image, const uint8_t* d_prm_u8, const int32_t* d_boxes,
                      const int64_t* d_offsets, int num_rois, int depth, int height, int width, int mode,
                      uint16_t* d_out_image, uint16_t* d_out_prm, void* stream);

/* Round 2: element-parallel forms of the two functions above, results identical.
 *   m3d_prm_quantize_windows_u8  the uint8 maps straight from the cone-cropped windows the back-propagation returns (d_windows
 *       [P, win^3] un-normalised, d_sums [P], d_origins int32 [P,3]): equals m3d_prm_quantize_u8 of the maps m3d_prm_scatter would
 *       build, without ever materialising them (tools/infer_simple.py:233-238).  d_ws: 16 * num_peaks bytes; on return
 *       int32 word 3 of each 16-byte record is 1 when the peak's uint8 map has a non-zero voxel.
 *   m3d_roi_normalize_ws         m3d_roi_normalize over a (chunks, RoI) grid; total_voxels = d_offsets[num_rois];
 *       d_ws: 24 * num_rois bytes. */
int m3d_prm_quantize_windows_u8(const float* d_windows, const float* d_sums, const int32_t* d_origins, int num_peaks, int win,
                                int depth, int height, int width, uint8_t* d_out, void* d_ws, size_t ws_bytes, void* stream);
/* Round 4: the same uint8 values as WINDOWS [P, win^3] (0 where a window voxel lies outside the tile) - what the whole-volume driver
 * sends to the host writer (m3d_io.h: m3d_tiff_encode_window_stack_u8) instead of the dense maps.  Same d_ws contract. */
int m3d_prm_quantize_windows_compact_u8(const float* d_windows, const float* d_sums, const int32_t* d_origins, int num_peaks, int win,
                                        int depth, int height, int width, uint8_t* d_out_windows, void* d_ws, size_t ws_bytes, void* stream);
int m3d_roi_normalize_ws(const uint16_t* d_image, const uint8_t* d_prm_u8, const int32_t* d_boxes, const int64_t* d_offsets,
                         int num_rois, int64_t total_voxels, int depth, int height, int width, int mode, uint16_t* d_out_image,
                         uint16_t* d_out_prm, void* d_ws, size_t ws_bytes, void* stream);
/* ... with an indirection and an optional compact source: RoI r reads map d_map_index[r] (int32 [num_rois]; NULL = map r) of d_prm_u8 =
 * the dense stack (win = 0) or the uint8 windows [*, win^3] of m3d_prm_quantize_windows_compact_u8 with d_win_origins int32 [*, 3] (a
 * map is zero outside its window): neither a gathered copy of the valid detections' maps nor the dense maps are needed. */
int m3d_roi_normalize_idx(const uint16_t* d_image, const uint8_t* d_prm_u8, const int32_t* d_map_index, int win,
                          const int32_t* d_win_origins, const int32_t* d_boxes, const int64_t* d_offsets, int num_rois,
                          int64_t total_voxels, int depth, int height, int width, int mode, uint16_t* d_out_image, uint16_t* d_out_prm,
                          void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Per-RoI 2D-Otsu binarisation.  Replaces otsu.otsu_py_2d_fast (tools/otsu.py:199-284) for uint16 inputs
 * (the callers normalise to uint16: tools/binarization_soma.py:85-91, binarization_nuclei.py:110-121).
 * A batch of `num_rois` independent crops: crop r occupies voxels [offsets[r], offsets[r+1]) of d_image /
 * d_prm / d_mask.  d_kb receives (k, b_max) per RoI; status[r] != 0 marks "no separating line".
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_otsu2d_workspace_bytes(int num_rois, int max_gray_range);
int m3d_otsu2d_batch(const uint16_t* d_image, const uint16_t* d_prm, const int64_t* d_offsets, int num_rois,
                     int max_gray_range, uint8_t* d_mask, int32_t* d_kb, int32_t* d_status, void* d_ws,
                     size_t ws_bytes, void* stream);

/* Volume pre-filters of tools/binarization_nuclei.py:44-45, bit-exact with SciPy 1.15 (uint16 volumes):
 *   m3d_gaussian_filter_u16  ndimage.gaussian_filter(img, sigma): separable correlate1d along z, y, x with 'reflect'
 *                            borders, fp64 accumulation in SciPy's order, truncation to uint16 after every pass.
 *                            d_weights: radius+1 doubles (centre first) computed by the host exactly as SciPy does;
 *                            d_tmp: scratch volume of the same size.
 *   m3d_median_filter3_u16   ndimage.median_filter(img, size=3): rank 13 of the 27 reflect-padded neighbours. */
int m3d_gaussian_filter_u16(const uint16_t* d_in, uint16_t* d_out, uint16_t* d_tmp, int depth, int height, int width,
                            const double* d_weights, int radius, void* stream);
int m3d_median_filter3_u16(const uint16_t* d_in, uint16_t* d_out, int depth, int height, int width, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Connected-component post-processing of the Otsu masks, batched per RoI (the step after Otsu: SURVEY 8f-2).
 * Crops are concatenated; crop r = voxels [d_offsets[r], d_offsets[r+1]) with dims d_dims[3r..3r+2] = (ez,ey,ex).
 *   m3d_cc_largest_batch   keep the largest 26-connected component (skimage.measure.label / cc3d default
 *                          connectivity; tools/binarization_soma.py:96-98, binarization_nuclei.py:125-130).
 *                          tie_last = 1: among equal sizes the highest label id (argsort(...)[-1], soma),
 *                          0: the lowest (np.argmax, nuclei).  invert = 1 runs on the complement and writes
 *                          255 everywhere except its largest component = hole filling (nuclei :132-137).
 *                          d_status[r] = 1 when there is no component at all, 2 for inconsistent dims / offsets,
 *                          3 if the label propagation did not converge within its sweep bound (output zeroed).
 *   m3d_binary_closing6_batch  scipy.ndimage.binary_closing defaults: 6-neighbourhood, 1 iteration, border 0
 *                          (binarization_nuclei.py:139).
 *   m3d_paint_instances    write d_ids[r] into the uint32 label volume wherever crop r (box int32 [R,6] inclusive)
 *                          is set and no SMALLER id covers the voxel == "paint only where still 0" in ascending
 *                          id order (binarization_soma.py:99-102).  The volume must be pre-filled with 0xFFFFFFFF.
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_cc_workspace_bytes(int64_t total_voxels);
int m3d_cc_largest_batch(const uint8_t* d_mask, const int64_t* d_offsets, const int32_t* d_dims, int num_rois,
                         int64_t total_voxels, int invert, int tie_last, uint8_t* d_out, int32_t* d_status,
                         void* d_ws, size_t ws_bytes, void* stream);
int m3d_binary_closing6_batch(const uint8_t* d_mask, const int64_t* d_offsets, const int32_t* d_dims, int num_rois,
                              int64_t total_voxels, uint8_t* d_out, void* d_ws, size_t ws_bytes, void* stream);
int m3d_paint_instances(const uint8_t* d_mask, const int64_t* d_offsets, const int32_t* d_boxes, const int32_t* d_ids,
                        int num_rois, int depth, int height, int width, uint32_t* d_volume, void* stream);
/* After the last m3d_paint_instances: sentinel 0xFFFFFFFF -> 0 and d_present[id] = 1 (uint8 [max_id + 1], caller zero-fills; may be
 * NULL) for every id in [1, max_id] that occurs in the volume (`mask_id in np.unique(seg)`, binarization_soma.py:103). */
int m3d_paint_finish(uint32_t* d_volume, int64_t num_voxels, int max_id, uint8_t* d_present, void* stream);
/* A tile's painting starts with ONE launch: the volume to the 0xFFFFFFFF sentinel, d_present [num_present] to 0 and the paint id of each
 * of the num_rois processed detections: d_ids[r] = d_idx[r] + first_id, or -1 (never paints) where the Otsu / component stage failed
 * (status != 0) or the detection's response map is all zero (d_map_stats: the workspace m3d_prm_quantize_windows*_u8 filled, 4 words
 * per map; null: not tested) - binarization_soma.py:74-76,94-98. */
int m3d_paint_begin(uint32_t* d_volume, int64_t num_voxels, uint8_t* d_present, int num_present, const int32_t* d_status_otsu,
                    const int32_t* d_status_cc, const int32_t* d_map_stats, const int64_t* d_idx, int num_rois, int first_id,
                    int32_t* d_ids, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Evaluation of instance-label volumes (csrc/eval3d.hip).  Replaces the voxel work of tools/evaluation/
 * eval_instance_segmentation_soma.py:186-199 (one bool mask per instance, then mask_iou.py:50-68 mask_iou_fast, a P x G x V loop)
 * and of evaluation_nuclei_f1score_seg.py:88-133 (pixel sums of the TP boxes).
 *   m3d_label_overlap   two label volumes d_a, d_b of num_voxels labels (label_bytes 2: uint16, 4: int32), labels in [0, max] with
 *                       max_a, max_b < 2^24 -> d_count_a [max_a + 1] / d_count_b [max_b + 1] int64 voxel counts per label, and the
 *                       pairs (a, b) with a > 0 and b > 0 that occur: d_pairs int32 [capacity, 2] sorted by (a, b), d_pair_counts
 *                       int64 [capacity] their voxel counts.  d_status int64 [2]: [0] flags (1: a label above its maximum - never
 *                       used as an index; 2: the hash table of `capacity` slots (a power of two) was full - re-launch with a larger
 *                       one; min(V, (max_a + 1)(max_b + 1)) pairs can occur), [1] the number of pairs.  Workspace
 *                       m3d_label_overlap_workspace_bytes(max_a, capacity).  Integer counts, sorted output: bit-identical run to run.
 *   m3d_label_iou_best  per row r (d_row_ids int32 [num_rows]: pred ids in score order; ids may be absent or > max_a = empty mask):
 *                       iou[r, c] = float32((double)inter / (double)(|a| + |b| - inter)) for GT column c = d_gt_col[b] (int32
 *                       [max_b + 1], -1 = not a column) -> d_max_iou fp32 [num_rows], d_argmax int32 [num_rows] (the lowest column of
 *                       the largest fp32 value; 0 for a row without overlap, as np.argmax of a zero row), d_iou fp32 [num_rows,
 *                       num_cols] the dense matrix (or NULL).  Inputs are m3d_label_overlap's outputs.
 *   m3d_box_union_overlap_counts  d_counts int64 [3] = Σ(pred > 0), Σ(gt > 0), Σ(pred > 0 & gt > 0 & inside at least one box) over
 *                       the [depth, height, width] volumes; d_ranges int32 [num_boxes, 6] = half-open (z0, z1, y0, y1, x0, x1), as
 *                       the host normalised them (clipped again here).  Boxes are painted into a coverage bit-mask (workspace
 *                       m3d_box_union_overlap_workspace_bytes), then one pass counts.
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_label_overlap_workspace_bytes(int max_a, int64_t capacity);
int m3d_label_overlap(const void* d_a, const void* d_b, int label_bytes, int64_t num_voxels, int max_a, int max_b, int64_t capacity,
                      int64_t* d_count_a, int64_t* d_count_b, int32_t* d_pairs, int64_t* d_pair_counts, int64_t* d_status, void* d_ws,
                      size_t ws_bytes, void* stream);
int m3d_label_iou_best(const int32_t* d_pairs, const int64_t* d_pair_counts, int64_t num_pairs, const int64_t* d_count_a, int max_a,
                       const int64_t* d_count_b, int max_b, const int32_t* d_gt_col, int num_cols, const int32_t* d_row_ids, int num_rows,
                       float* d_max_iou, int32_t* d_argmax, float* d_iou, void* stream);
size_t m3d_box_union_overlap_workspace_bytes(int64_t num_voxels);
int m3d_box_union_overlap_counts(const void* d_pred, const void* d_gt, int label_bytes, int depth, int height, int width,
                                 const int32_t* d_ranges, int num_boxes, int64_t* d_counts, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Whole-volume connected-component labelling and sphere painting (csrc/label3d.hip): the voxel work of the two baselines of
 * tools/evaluation/eval_instance_segmentation_soma_ngps.py (DSN :184-187 skimage.measure.label, NGPS :159-183 spheres).
 *   m3d_label_components   d_in: a [depth, height, width] volume of in_bytes 1 (uint8), 2 (uint16) or 4 (int32); connectivity 6, 18
 *                          or 26.  A component is a maximal connected set of voxels sharing one NON-ZERO value (skimage.measure.label
 *                          defaults: equal values connect; 0 is background and gets label 0).  d_labels int32, same shape: 1..K in the
 *                          raster order (z, y, x) of each component's first voxel, as skimage / cc3d / scipy.ndimage.label number them;
 *                          *d_num = K (device).  The output is a function of the input alone: bit-identical run to run.  Workspace
 *                          m3d_label_components_workspace_bytes(num_voxels).  depth * height * width >= 2^31: M3D_EUNSUPPORTED before
 *                          any launch (parents are int32); an empty dimension, other in_bytes or connectivity: M3D_EINVAL.
 *   m3d_label_counts       d_counts int64 [num_labels + 1] = voxels per label of an int32 label volume (zero-filled by the call;
 *                          labels outside [0, num_labels] are not counted).  Runs of equal labels are folded before any atomic.
 *   m3d_paint_spheres      d_spheres int32 [num_spheres, 4] = (x, y, z, r); sphere i (0-based) paints id i + 1 into the uint16
 *                          [depth, height, width] volume over ix in [max(1, x - r), min(width, x + r + 1)), likewise y / height and
 *                          z / depth, where (ix-x)^2 + (iy-y)^2 + (iz-z)^2 <= r^2, only when r >= 6.  Index 0 of every axis is never
 *                          painted (the script's clamp).  Where spheres overlap the highest index wins (the script's overwrite order),
 *                          whatever order the launches run in.  The volume is written whole.  num_spheres > 65535: M3D_EINVAL (the
 *                          script would wrap in its uint16 array).  Workspace m3d_paint_spheres_workspace_bytes(num_voxels).
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_label_components_workspace_bytes(int64_t num_voxels);
int m3d_label_components(const void* d_in, int in_bytes, int depth, int height, int width, int connectivity, int32_t* d_labels,
                         int32_t* d_num, void* d_ws, size_t ws_bytes, void* stream);
int m3d_label_counts(const int32_t* d_labels, int64_t num_voxels, int num_labels, int64_t* d_counts, void* stream);
size_t m3d_paint_spheres_workspace_bytes(int64_t num_voxels);
int m3d_paint_spheres(const int32_t* d_spheres, int num_spheres, int depth, int height, int width, uint16_t* d_volume, void* d_ws,
                      size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * RPN training step (csrc/rpn_train.hip): what lib/roi_data/rpn.py:120-279 (_get_rpn_blobs) does on the host per sample and
 * lib/modeling/rpn_heads.py:140-170 (single_scale_rpn_losses, sigmoid branch) + lib/utils/net.py:15-32 (smooth L1, beta 1/9) do
 * with its four dense blobs.  Single-scale (no FPN).  The anchor field is the wide cube of data_utils.py:50-102: field_size^3
 * positions (z-major, x-minor), num_cell_anchors anchors each, anchor = fp64 cell anchor + position * stride, rounded to fp32;
 * "flat field index" i = position * A + a.  A "wide index" addresses the [A, F, F, F] blob of rpn.py:260-261: a * F^3 + position.
 * Limits: A <= 64, F^3 A < 2^32 - 1024, batch_per_im <= 4096 (M3D_EUNSUPPORTED beyond, before any launch).
 *   m3d_rpn_targets   cell_anchors: HOST fp64 [A, 6].  d_gt fp32 [num_gt, 6], d_dc fp32 [num_dc, 6] ("don't care" boxes, may be NULL
 *                     with num_dc 0).  Inside test of rpn.py:124-140 (straddle_thresh < 0: every anchor).  IoU as
 *                     m3d_bbox_overlaps3d.  fg (rpn.py:169-177): IoU equal (fp32) to its box's maximum over the inside anchors - a
 *                     box that overlaps no inside anchor has maximum 0 and so makes every inside anchor with IoU 0 fg, as in the
 *                     reference - or maximum IoU >= positive_overlap.  Thresholds are compared as fp32 (NumPy 2 compares an fp32
 *                     array with a Python scalar in fp32).  Sampling is a pure function of `seed`: with fin() the splitmix64
 *                     finaliser (x * 0x9E3779B97F4A7C15, two xor-shift-multiplies, a last xor-shift), stream = fin(seed) and
 *                     key(i) = upper 32 bits of fin(stream + i), so that consecutive seeds give unrelated draws.
 *                     If more than num_fg anchors are fg, the num_fg with the smallest
 *                     (key(flat field index), flat field index) stay (rpn.py:189-196).  bg candidates (rpn.py:202-203): inside,
 *                     maximum IoU < negative_overlap against d_gt and against d_dc, n of them in ascending field order; only if
 *                     n > num_bg = batch_per_im - #fg, draw j = 0 .. num_bg-1 labels candidate (key(2^40 + j) * n) >> 32 as bg
 *                     (with replacement; a draw that hits a sampled fg anchor turns it into bg, rpn.py:204-206).  num_gt = 0 (the
 *                     reference raises NameError): no fg, every inside anchor is a candidate unless a d_dc box excludes it.
 *                     Outputs (device): d_fg_index int64 [num_fg] / d_bg_index int64 [batch_per_im]: wide indices of the anchors
 *                     labelled 1 / 0, ascending, -1 beyond the count; d_target_index int64 [num_fg] + d_targets fp32 [num_fg, 6]:
 *                     the fg set as sampled BEFORE the bg draws and its bbox_transform_inv_3d targets against the first-argmax box
 *                     (boxes_3d.py:228-270, unit weights; dx,dy,dz fp32 in the reference's operation order, dw,dh,ds = fp32(log in
 *                     fp64)), rows beyond the count -1 / 0; d_counts int64 [8] = #fg, #bg, #target rows, num_examples (rpn.py:229),
 *                     inside anchors, fg before sampling, bg candidates, bg draws.  Integer atomics and value-ordered selection only:
 *                     bit-identical run to run.  Workspace m3d_rpn_targets_workspace_bytes(A, F, num_gt, batch_per_im, num_fg).
 *   m3d_rpn_targets_wide  expands one image's outputs into the reference's dense blobs (rpn.py:260-278): d_labels int32 [A,F,F,F]
 *                     (-1 / 0 / 1), d_targets_wide, d_inside_wide, d_outside_wide fp32 [6A,F,F,F] (channel 6 a + component);
 *                     outside weight = fp32(1.0 / num_examples) on labels 0 and 1, inside weight 1 on label 1 (rpn.py:219-231).
 *   m3d_rpn_loss      d_cls_logits fp32 [B,A,s,h,w], d_bbox_pred fp32 [B,6A,s,h,w]; the targets of the B images stacked:
 *                     d_fg_index [B,num_fg], d_bg_index [B,batch_per_im], d_target_index [B,num_fg], d_targets [B,num_fg,6],
 *                     d_counts [B,8].  Only sampled anchors inside the crop [:s,:h,:w] of the field count (rpn_heads.py:145-150).
 *                     d_losses fp32 [2] = loss_cls = sum bce_with_logits / W with W = labelled in-crop anchors over the batch (0 if
 *                     W = 0, where the reference divides 0 by 0), loss_bbox = sum out * smoothL1(p - t) / B.  d_grad_logits /
 *                     d_grad_pred (input shapes, written whole): (sigmoid(x) - y) / W and out * clamp((p - t) / beta, -1, 1) / B at
 *                     those anchors, exactly 0 elsewhere.  One workgroup, fixed summation tree: bit-identical run to run.
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_rpn_targets_workspace_bytes(int num_cell_anchors, int field_size, int num_gt, int batch_per_im, int num_fg);
int m3d_rpn_targets(const double* cell_anchors, int num_cell_anchors, int field_size, int stride, const float* d_gt, int num_gt,
                    const float* d_dc, int num_dc, double im_slices, double im_height, double im_width, double straddle_thresh,
                    double positive_overlap, double negative_overlap, int batch_per_im, int num_fg, uint64_t seed,
                    int64_t* d_fg_index, int64_t* d_bg_index, int64_t* d_target_index, float* d_targets, int64_t* d_counts,
                    void* d_ws, size_t ws_bytes, void* stream);
int m3d_rpn_targets_wide(const int64_t* d_fg_index, const int64_t* d_bg_index, const int64_t* d_target_index, const float* d_targets,
                         const int64_t* d_counts, int num_cell_anchors, int field_size, int num_fg, int batch_per_im,
                         int32_t* d_labels, float* d_targets_wide, float* d_inside_wide, float* d_outside_wide, void* stream);
int m3d_rpn_loss(const float* d_cls_logits, const float* d_bbox_pred, int batch, int num_cell_anchors, int slices, int height, int width,
                 int field_size, const int64_t* d_fg_index, const int64_t* d_bg_index, const int64_t* d_target_index,
                 const float* d_targets, const int64_t* d_counts, int num_fg, int batch_per_im, float* d_losses, float* d_grad_logits,
                 float* d_grad_pred, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Box-head training step (csrc/box_head_train.hip): what GenerateProposalLabelsOp_3d does on the host in the middle of every
 * training step - add_proposals (lib/datasets/nuclei_dataset.py:429-547), _sample_rois (lib/roi_data/fast_rcnn.py:129-248) - and
 * fast_rcnn_losses (lib/modeling/fast_rcnn_heads.py:50-66, smooth L1 with beta 1, lib/utils/net.py:15-32) do with its five blobs.
 * Image scale 1, no FPN.  The "roidb rows" of image b are r = 0 .. K_b-1 for its ground-truth boxes in the given order, then
 * r = K_b .. for its proposals in order.
 * Limits (M3D_EUNSUPPORTED, before any launch): num_classes <= 64, batch_per_im <= 4096, num_images <= 64, max K_b + rows < 2^31 - 256,
 * cls_agnostic_bbox_reg != 0 (not implemented: in the reference it also clips the classification labels, fast_rcnn.py:217).
 *   m3d_box_head_targets  all num_images images in one launch pair.  d_gt fp32 [sum K_b, 6]: the images' boxes one after another,
 *                     gt_offsets HOST int32 [num_images + 1] (gt_offsets[0] = 0; image b owns [gt_offsets[b], gt_offsets[b+1])),
 *                     d_gt_classes int32 [sum K_b] in 1 .. num_classes-1 (NULL: all 1), d_gt_crowd uint8 [sum K_b] (NULL: none).
 *                     d_rois fp32 [num_images, rows, 7] and d_num int32 [num_images] exactly as m3d_generate_proposals3d_batched
 *                     leaves them: image b's proposals are d_rois[b, :num[b], 1:7], column 0 is ignored.  Labelling: a non-crowd
 *                     gt row has overlap 1, its own class and is assigned to itself; a crowd gt row has overlap -1; a proposal row
 *                     takes the IoU (as m3d_bbox_overlaps3d) against the non-crowd boxes, is assigned to the FIRST arg-max and has
 *                     that box's class if the maximum is > 0, else overlap 0, class 0, no assignment.  fg candidates: overlap >=
 *                     fg_thresh; bg candidates: bg_thresh_lo <= overlap < bg_thresh_hi (compared as fp32).  Sampling (stream =
 *                     fin(seeds[b]), key(i) = upper 32 bits of fin(stream + i), fin = the splitmix64 finaliser as for
 *                     m3d_rpn_targets; seeds HOST uint64 [num_images]): the min(fg_per_im, #fg candidates) candidates with the
 *                     smallest (key(r), r) stay, then the min(batch_per_im - #fg kept, #bg candidates) bg candidates with the
 *                     smallest (key(2^40 + r), r); both without replacement.  Outputs (device, per image padded to batch_per_im,
 *                     fg rows ascending in r, then bg rows ascending in r): d_rows int64 [num_images, batch] (-1 beyond the count),
 *                     d_labels int32 (class of an fg row, 0 for bg, -1 beyond), d_out_rois fp32 [.., 6] (0 beyond), d_targets fp32
 *                     [.., 6]: bbox_transform_inv_3d (boxes_3d.py:228-268) of an fg row against its assigned box with
 *                     bbox_reg_weights (HOST fp64 [6]): dx,dy,dz fp32 in the reference's operation order, dw,dh,ds =
 *                     fp32(weight * log in fp64 of the fp32 ratio); 0 on bg rows and beyond.  d_counts int64 [num_images, 8] = rows
 *                     sampled, fg sampled, bg sampled, fg candidates, bg candidates, crowd gt rows, non-crowd gt boxes, proposals.
 *                     Integer atomics and value-ordered selection only: bit-identical run to run.
 *                     Workspace m3d_box_head_targets_workspace_bytes(num_images, max K_b, rows).
 *   m3d_box_head_target_blobs  _expand_bbox_targets (fast_rcnn.py:222-248): d_labels [num_rows], d_targets [num_rows, 6] (any number
 *                     of stacked images) -> d_bbox_targets, d_inside_weights, d_outside_weights fp32 [num_rows, 6 num_classes]:
 *                     the row's targets / 1 / 1 in slots 6 label .. 6 label + 5 of rows with label > 0, 0 elsewhere.
 *   m3d_box_head_loss  d_cls_score fp32 [B batch, C], d_bbox_pred fp32 [B batch, 6 C]; d_labels, d_targets, d_counts of the B images
 *                     stacked.  R = sum of the sampled-row counts (device side).  d_losses fp32 [3] = loss_cls = sum softmax cross
 *                     entropy / R, loss_bbox = sum over fg rows and slots 6 label + j of smoothL1(p - t) / R, accuracy_cls = rows
 *                     whose first arg-max is the label / R; zeros if R = 0.  Row terms in fp64 from the fp32 inputs, one workgroup,
 *                     fixed summation tree, each result rounded once.  d_grad_score / d_grad_pred (input shapes, written whole):
 *                     (softmax - onehot) / R at labelled rows, clamp(p - t, -1, 1) / R at the six slots of fg rows, exactly 0
 *                     elsewhere.
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_box_head_targets_workspace_bytes(int num_images, int max_gt, int rows);
int m3d_box_head_targets(const float* d_gt, const int32_t* d_gt_classes, const uint8_t* d_gt_crowd, const int32_t* gt_offsets,
                         int num_images, const float* d_rois, const int32_t* d_num, int rows, int batch_per_im, int fg_per_im,
                         double fg_thresh, double bg_thresh_hi, double bg_thresh_lo, const double* bbox_reg_weights, int num_classes,
                         int cls_agnostic_bbox_reg, const uint64_t* seeds, int64_t* d_rows, int32_t* d_labels, float* d_out_rois,
                         float* d_targets, int64_t* d_counts, void* d_ws, size_t ws_bytes, void* stream);
int m3d_box_head_target_blobs(const int32_t* d_labels, const float* d_targets, int64_t num_rows, int num_classes,
                              float* d_bbox_targets, float* d_inside_weights, float* d_outside_weights, void* stream);
int m3d_box_head_loss(const float* d_cls_score, const float* d_bbox_pred, const int32_t* d_labels, const float* d_targets,
                      const int64_t* d_counts, int num_images, int batch_per_im, int num_classes, float* d_losses,
                      float* d_grad_score, float* d_grad_pred, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Mask-branch training step (csrc/mask_train.hip; DESIGN, "Mask-branch training targets"): what add_mask_rcnn_blobs
 * (lib/roi_data/mask_rcnn.py:34-135) does on the host for every sampled fg RoI - a volume filled in Python, skimage's resize, a
 * threshold - and mask_rcnn_losses (lib/modeling/mask_rcnn_heads.py:90-99).  With the resize carried out in fp64, "resize > 0" is a set
 * predicate: output (i,j,k) is set iff a source voxel is set inside F_s(i) x F_h(j) x F_w(k), F_n(i) = [lo, hi] the source indices
 * whose weight at output i is not 0 (Gaussian radius int(4 sigma + 0.5), sigma = max(0, (n / M - 1) / 2), none for sigma <= 1e-15;
 * order-1 corners of the fp64 coordinate n / M (i + 0.5) - 0.5, the upper one only with a weight that is not exactly 0; mirror
 * boundary).  That is what is computed.  The reference's resize writes fp32 and loses products below 2^-150: on extents where a corner
 * weight is about 2e-15 (M = 14: 18, 34, 58, 82, ... - 42 lengths up to 1024) the result can hold voxels, on that corner's output index,
 * which the reference leaves 0; never fewer (DESIGN).
 *   m3d_mask_targets  d_labels int32 [B, batch], d_rois fp32 [B, batch, 6], d_counts int64 [B, 8]: the stacked outputs of
 *                     m3d_box_head_targets; the fg rows of image b are its first min(counts[b][1], fg_per_im) rows.  gt_offsets HOST
 *                     int32 [B + 1], d_gt_classes int32 / d_gt_crowd uint8 [sum K] (NULL: all 1 / none) as for m3d_box_head_targets.
 *                     Per fg row: the IoU (m3d_bbox_overlaps3d) against the boxes of the image's objects with class > 0 that are not
 *                     crowd, in their order; the FIRST arg-max is the row's object (all-zero IoUs: the first such object; no such
 *                     object: index -1 and an all-zero target).
 *                     mode M3D_MASK_SPOT: d_spots fp32 [sum K, 4] = (x, y, z, r) in tile coordinates, in_size HOST int32 [3] =
 *                     TRAIN.IN_SIZE (slices, height, width).  Boxes: spots_to_boxes (segms.py:209-225), c -+ (r - 1) in fp32 clipped
 *                     to [0, IN_SIZE - 1].  Target: spot_to_mask_wrt_box (segms.py:120-150): extents int(max(hi - lo, 2)) of the fp32
 *                     RoI (no + 1), centre sp - lo in fp32, voxel set iff ((i - z)^2 + (j - y)^2) + (k - x)^2 < r^2 in fp32 (strict)
 *                     for some integer point of the footprint box - decided at the per-axis nearest integers.
 *                     mode M3D_MASK_LABELS: d_gt fp32 [sum K, 6] the roidb boxes, d_markers int32 [sum K], images HOST [B]: per image
 *                     the device label volume [depth, height, width] in tile coordinates, dtype 0 = uint16, 1 = int32.  Target:
 *                     rle_to_mask_wrt_box (segms.py:152-193) with mask_gt = (label == marker): both boxes truncated towards zero,
 *                     extent max(hi - lo, 2) of the integer RoI, copied region [max(lo), min(hi)) per axis (cut to the extent and to
 *                     the volume, so every read lies inside it; an empty intersection copies nothing, where the reference raises),
 *                     then the interval-"any" along x, y and z, one read per label.
 *                     RoI extents are clamped to [2, 1024] on the device before any size is derived from them.
 *                     Outputs (device, fixed shapes, written whole): d_masks int32 [B, fg_per_im, Cm M^3], z-major as
 *                     np.reshape(mask, M**3), Cm = cls_specific ? num_classes : 1; with cls_specific every slot outside the row's
 *                     class block is -1 (_expand_to_class_specific_mask_targets); rows beyond the fg count are all -1.
 *                     d_mask_rois fp32 [B, fg_per_im, 6] (0 beyond), d_assign int32 [B, fg_per_im] the object's index within the
 *                     image (-1 beyond), d_mask_counts int64 [B, 4] = fg rows, positive voxels, labelled voxels, 0.
 *                     One launch; integer logic and integer atomics only: bit-identical run to run.  No workspace.
 *   m3d_mask_loss     d_mask_pred fp32 [num_rois, mask_classes, M, M, M], d_masks int32 of the same element count.  W = the number
 *                     of targets > -1, counted on the device (d_num int64 [1], may be NULL).  d_loss fp32 [1] = weight_loss_mask *
 *                     sum over t > -1 of (max(x, 0) - x t + log1p(exp(-|x|))) / W; d_grad (input shape, written whole) =
 *                     weight_loss_mask (sigmoid(x) - t) / W at labelled elements, exactly 0 elsewhere.  W = 0 (the reference divides
 *                     0 by 0): loss 0 and an all-zero gradient.  Terms in fp64 from the fp32 inputs; one partial sum per chunk of
 *                     4096 elements (fixed tree), a finish kernel adds them in ascending order; each result rounded once; no
 *                     floating-point atomics.  Workspace m3d_mask_loss_workspace_bytes(num_rois, mask_classes, M), 8-byte aligned.
 * Limits, checked before any device pointer is followed or anything is launched.  M3D_EINVAL: a NULL or misaligned pointer, M < 2,
 * fg_per_im < 1, batch_per_im < 1, num_images < 1, num_classes < 2, another mode, another label dtype, descending offsets, in mask mode
 * an image without objects (the sampler's counts are not read on the host, so every image may hold fg rows) or without a volume.
 * M3D_EUNSUPPORTED: num_images > 64, M > 32, num_classes > 64, fg_per_im > 4096, K > 2048 in an image, 2^31 loss elements or more.
 * ------------------------------------------------------------------------------------------------------- */
#define M3D_MASK_SPOT 0
#define M3D_MASK_LABELS 1
typedef struct { const void* labels; int dtype, depth, height, width; } m3d_mask_image;
int m3d_mask_targets(const int32_t* d_labels, const float* d_rois, const int64_t* d_counts, int num_images, int batch_per_im,
                     int fg_per_im, int resolution, int num_classes, int cls_specific, int mode, const int32_t* gt_offsets,
                     const int32_t* d_gt_classes, const uint8_t* d_gt_crowd, const float* d_spots, const int32_t* in_size,
                     const float* d_gt, const int32_t* d_markers, const m3d_mask_image* images, int32_t* d_masks, float* d_mask_rois,
                     int32_t* d_assign, int64_t* d_mask_counts, void* stream);
size_t m3d_mask_loss_workspace_bytes(int64_t num_rois, int mask_classes, int resolution);
int m3d_mask_loss(const float* d_mask_pred, const int32_t* d_masks, int64_t num_rois, int mask_classes, int resolution,
                  double weight_loss_mask, float* d_loss, int64_t* d_num, float* d_grad, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * BatchNorm3d on batch statistics (csrc/bn_train.hip): what nn.BatchNorm3d -> nnf.relu -> nn.MaxPool3d(2, 2) of lib/modeling/DSN.py:19-68
 * do under maskRCNN.train(), forward and backward.  d_x fp32 contiguous [batch, channels, depth, height, width]; V = depth height width
 * values per (image, channel) slab, n = batch V values per channel.  Every sum runs in fp64 over spans of one slab whose boundaries
 * depend on the shape only, a fixed tree per workgroup and an ascending loop over the spans; no floating-point atomics: bit-identical
 * run to run.  DESIGN ("BatchNorm training") has the contract in full.
 * Limits, checked before any pointer is read or anything is launched: channels <= 4096, n < 2^31 and batch channels ceil(V / 4096) <
 * 2^24 (the largest grid stays under the 2^32 threads of one launch; M3D_EUNSUPPORTED beyond); n >= 2 where batch statistics are taken
 * (m3d_bn_stats, m3d_bn_backward with training != 0), even depth, height and width with pool != 0 (M3D_EINVAL).  Workspace: with d_ws == NULL a call launches nothing and stores the bytes it needs in *ws_bytes; otherwise *ws_bytes
 * is the capacity of d_ws (8-byte aligned; M3D_EWORKSPACE if too small).
 *   m3d_bn_stats     d_mean = fp32(S1 / n), d_var = fp32(max(S2 / n - (S1 / n)^2, 0)) (biased), d_invstd = fp32(1 / sqrt(fp64(d_var) +
 *                    eps)), fp32 [channels] each; S1, S2 = fp64 sums of x and of the exact fp64 squares.  d_running_mean /
 *                    d_running_var (fp32 [channels], each may be NULL) are updated in place as torch.nn.BatchNorm3d updates them:
 *                    rm <- fp32((1 - momentum) rm + momentum mean), rv <- fp32((1 - momentum) rv + momentum var n / (n - 1)), in fp64
 *                    from the unrounded batch statistics.
 *   m3d_bn_invstd    d_invstd of given variances by the same expression (evaluation mode: the running variance).
 *   m3d_bn_apply     z = (x - mean) * a + beta in fp32 without contraction, a = fp32(gamma * invstd); y = relu ? max(z, 0) : z.
 *                    pool == 0: d_y has d_x's shape.  pool != 0: only the 2x2x2 max-pooled y [.., depth/2, height/2, width/2] and its
 *                    uint8 arg-max (z*4 + y*2 + x, first maximum, NaN propagates: m3d_maxpool3d_2x_forward's convention) are written.
 *                    d_mean / d_invstd are the batch statistics, or the running mean and m3d_bn_invstd of the running variance.
 *   m3d_bn_backward  d_grad_out has d_y's shape (pooled with pool != 0, then d_argmax is m3d_bn_apply's).  Effective gradient of a
 *                    voxel: g = d_grad_out (pool: of its window if it is the window's arg-max, else 0), 0 where relu and not z > 0,
 *                    z recomputed as in m3d_bn_apply.  d_grad_beta = fp32(sum g), d_grad_gamma = fp32(sum g xhat) with xhat =
 *                    fp32((x - mean) * invstd), summed in fp64.  training != 0: d_grad_x = a ((g - k1) - xhat k2), k1 = fp32(sum g /
 *                    n), k2 = fp32(sum g xhat / n); training == 0: d_grad_x = a g.
 * ------------------------------------------------------------------------------------------------------- */
int m3d_bn_stats(const float* d_x, int batch, int channels, int depth, int height, int width, double eps, float* d_running_mean,
                 float* d_running_var, double momentum, float* d_mean, float* d_var, float* d_invstd, void* d_ws, size_t* ws_bytes,
                 void* stream);
int m3d_bn_invstd(const float* d_var, int channels, double eps, float* d_invstd, void* stream);
int m3d_bn_apply(const float* d_x, const float* d_mean, const float* d_invstd, const float* d_gamma, const float* d_beta, int batch,
                 int channels, int depth, int height, int width, int relu, int pool, float* d_y, uint8_t* d_argmax, void* stream);
int m3d_bn_backward(const float* d_x, const float* d_mean, const float* d_invstd, const float* d_gamma, const float* d_beta,
                    const float* d_grad_out, const uint8_t* d_argmax, int batch, int channels, int depth, int height, int width,
                    int relu, int pool, int training, float* d_grad_x, float* d_grad_gamma, float* d_grad_beta, void* d_ws,
                    size_t* ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The solver's parameter update (csrc/sgd.hip): torch.optim.SGD with momentum and weight decay as tools/train_net_step.py:316-331 builds
 * it, over a whole parameter list in one launch, with the momentum-buffer scale of _CorrectMomentum (lib/utils/net.py:86-99) folded in.
 * `tensors` is a HOST array of `count` descriptors: p, g, m device fp32 [n], each tensor with its own lr and wd.  Per element, in fp32,
 * every operation rounded once and nothing contracted:
 *     c = mscale m ;  d = (wd == 0) ? g : g + wd p ;  m' = momentum c + d ;  p' = p - lr m'
 * p and m are updated in place, g is never written.  m == NULL is allowed only with momentum == 0: p' = p - lr d.  A zero-filled m on the
 * first step gives torch's "first step: buf = grad"; mscale == 1 is exact.  The descriptors travel as kernel arguments (64 per launch; a
 * longer list takes several launches): a step makes no host-to-device copy, no allocation and no host synchronisation.  Work is cut into
 * chunks of m3d_sgd_chunk() elements of one tensor, a function of the sizes and their order only.  16-byte accesses from the first common
 * 16-byte boundary of a chunk; a tensor whose pointers differ modulo 16 is updated element by element.
 * d_stats (NULL, or device fp64 [2], 8-byte aligned): d_stats[0] = sum of g^2 over the raw gradients of the call in fp64 (the fp64 square
 * of an fp32 value is exact), d_stats[1] = the number of non-finite gradient elements.  One partial and one count per chunk go to the
 * workspace (16 bytes per chunk); a finish kernel adds them in a fixed order (thread t of 256 the partials t, t + 256, ... ascending in
 * the call's chunk order, then a fixed tree): no floating-point atomics, bit-identical run to run for the same sizes, order, values and
 * pointer residues modulo 16, however many launches the call takes.
 * Workspace: ws_bytes != NULL with d_ws == NULL stores the bytes the call needs in *ws_bytes (0 with d_stats == NULL) and launches
 * nothing; otherwise *ws_bytes is the capacity of d_ws (8-byte aligned; M3D_EWORKSPACE if too small).  Without d_stats both may be NULL.
 * Limits, checked before any device pointer is followed or anything is launched: count < 0, n < 0, m == NULL with momentum != 0, a
 * NULL or not 4-byte aligned pointer, overlapping p / g / m ranges of one tensor: M3D_EINVAL; count > 65536, n >= 2^40:
 * M3D_EUNSUPPORTED.  count == 0 and tensors with n == 0 (whose pointers are not looked at) are legal and do nothing.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct { float* p; const float* g; float* m; long long n; float lr; float wd; } m3d_sgd_tensor;
int m3d_sgd_chunk(void);
int m3d_sgd_step(const m3d_sgd_tensor* tensors, int count, float momentum, float mscale, double* d_stats, void* d_ws, size_t* ws_bytes,
                 void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The solver's other optimiser and the gradient clip (csrc/adam.hip; m3d_sgd_step_scaled in csrc/sgd.hip).  Chunking, descriptor
 * passing, 16-byte accesses, statistics, workspace convention and the M3D_EUNSUPPORTED cases are those of m3d_sgd_step.
 *
 * m3d_adam_step: the single-tensor torch.optim.Adam of torch 2.10 (amsgrad and maximize off, coupled weight decay, betas = (beta1,
 * beta2)) which tools/train_net_step.py:330-333 builds, over a whole parameter list, 64 descriptors per launch.  `tensors` is a HOST
 * array of `count` descriptors: p, g, m (exp_avg), v (exp_avg_sq) device fp32 [n], and per tensor the two scalars of its step count t,
 * which the caller computes in doubles as torch does and rounds to fp32: lr_step = lr / (1 - beta1^t), bc2_sqrt = (1 - beta2^t)^0.5.
 * 1 - beta1, beta2, 1 - beta2 and eps are rounded to fp32 from the doubles given here, again as torch rounds them.  Per element, in
 * fp32, every operation rounded once, nothing contracted, square root and division correctly rounded:
 *     d = s g  (only with d_gscale) ;  d = (wd == 0) ? d : d + wd p ;  m' = m + (1 - beta1) (d - m) ;
 *     v' = beta2 v + (1 - beta2) (d d) ;  q = sqrt(v') / bc2_sqrt + eps ;  p' = p - lr_step (m' / q)
 * p, m and v are updated in place, g is never written.  Zero-filled m and v with the scalars of t = 1 give torch's first step.
 * d_gscale: NULL, or a device fp32 scalar s that the kernel reads (never a host value): the clip coefficient of m3d_grad_clip_coef.
 * d_stats as in m3d_sgd_step: the statistics of the RAW gradients.  A thread adds its squares in the order of m3d_sgd_step's 16-byte
 * path for the residue modulo 16 of g, also where p, m or v lie at another residue and the chunk is updated element by element: the two
 * numbers are a function of the sizes, order, values and pointer residues of the gradients alone, and equal m3d_grad_clip_coef's.
 * Limits, checked before any device pointer is followed: the rules of m3d_sgd_step for the four pointers (NULL, alignment, overlap of
 * any two of p, g, m, v); beta1 or beta2 outside [0, 1); eps not positive as fp32; bc2_sqrt outside (0, 1]; a misaligned d_gscale:
 * M3D_EINVAL.
 *
 * m3d_grad_clip_coef: clip_gradient of lib/utils/net.py:35-47 as a device scalar.  A read-only pass over the gradients (`tensors`: a
 * HOST array of {g, n}) that writes the two statistics to d_stats (required) and
 *     *d_coef = (float)(clip_norm / max(sqrt(d_stats[0]), clip_norm)),   square root and division in fp64,
 * 1.0f exactly when the norm does not exceed clip_norm.  The norm is the fp64 sum the solver defines; the reference adds per-parameter
 * fp32 norms on the host.  max() keeps a NaN norm, as Python's does there: a NaN gradient makes the coefficient NaN, an infinite one
 * makes it 0 and the scaled element NaN; d_stats[1] is the guard.  Limits: the rules of m3d_sgd_step for g; clip_norm not positive or
 * not finite, d_stats or d_coef NULL or misaligned: M3D_EINVAL.
 *
 * m3d_sgd_step_scaled: m3d_sgd_step with d = s g in front of the decay term, s read from d_gscale on the device; the statistics stay
 * those of the raw gradients.  d_gscale == NULL runs the kernels of m3d_sgd_step.
 *
 * A clipped step is the coefficient pass (one launch per 64 tensors and the finish) followed by the update (one launch per 64 tensors,
 * d_stats == NULL): no host read, allocation or copy, so it can be captured into a graph.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct { float* p; const float* g; float* m; float* v; long long n; float lr_step; float bc2_sqrt; float wd; } m3d_adam_tensor;
typedef struct { const float* g; long long n; } m3d_grad_tensor;
int m3d_adam_step(const m3d_adam_tensor* tensors, int count, double beta1, double beta2, double eps, const float* d_gscale,
                  double* d_stats, void* d_ws, size_t* ws_bytes, void* stream);
int m3d_grad_clip_coef(const m3d_grad_tensor* tensors, int count, double clip_norm, double* d_stats, float* d_coef, void* d_ws,
                       size_t* ws_bytes, void* stream);
int m3d_sgd_step_scaled(const m3d_sgd_tensor* tensors, int count, float momentum, float mscale, const float* d_gscale, double* d_stats,
                        void* d_ws, size_t* ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Training samples (train_sample.hip; DESIGN, "Training samples"): the minibatch of lib/roi_data/minibatch.py built on the device from
 * volumes that stay resident there - prep_im_for_blob(..., 'train') and crop_data_3d of lib/utils/blob.py:97-202.
 * `images` is a HOST array of `count` descriptors (they travel as kernel arguments): the device volume [depth,height,width] (dtype 0 =
 * uint16, 1 = float32), the device pointer to its mean, std, count (m3d_norm1_stats), its device boxes fp32 [num_boxes,6]
 * (x1,y1,z1,x2,y2,z2) and start_max (x, y, z) = min(floor(min over boxes of the lower coordinate), dim - in_size) of blob.py:106-114.
 * in_size: host (slices, height, width) of the crop.  seeds: host, one per image.  fixed_origin: NULL, or host [count,3] (x, y, z).
 * Search (one workgroup per image; need_crop != 0, no fixed_origin): per axis a (0 = x, 1 = y, 2 = z) the start is 0 where start_max[a]
 * == 0, else (key(a) * (start_max[a] + 1)) >> 32 with key(a) = mix_key(seed_stream(seed), a) of the sampling contract; the candidates of
 * an axis are range(start, dim - size, size / 2) followed by dim - size; candidates are numbered z outer, y, x inner.  A candidate's score
 * is the sum, in box order and in fp64, of ((x2 - x1) + 1)((y2 - y1) + 1)((z2 - z1) + 1) over the boxes that stay non-degenerate (no
 * lower coordinate equal to its upper one) after the fp32 shift and clip min(max(b - o, 0), size - 1); the differences are taken in fp64
 * from the fp32 coordinates.  The first strict maximum wins; no candidate above 0: status 1 and candidate 0.  The reference sums the
 * volumes in fp32: the same choice while all coordinates are integers and the sum stays below 2^24.  With fixed_origin the one candidate
 * is that origin.  need_crop == 0: origin 0, boxes pass through unshifted and unfiltered, 0 candidates, score 0.
 * Outputs (device): d_data fp32 [count, in_size] = ((float)x - (float)mean) / (float)std at every voxel of the crop, the arithmetic of
 * m3d_norm1 with f32_arith = 1, in 16-byte stores wherever a row of the output allows them; d_boxes fp32 [count,max_boxes,6] the kept
 * boxes shifted and clipped, in order, rows beyond the count 0; d_keep int32 [count,max_boxes] their source indices ascending, -1
 * beyond; d_info int32 [count,8] = ox, oy, oz, kept, status, candidates, 0, 0; d_score fp64 [count] the winner's volume.
 * Two launches, no host synchronisation, allocation or copy; integer and value-ordered selection only: bit-identical run to run.
 * Workspace: the convention of m3d_sgd_step (the call needs 0 bytes; d_ws and ws_bytes may be NULL).
 * Limits, checked before any device pointer is followed or anything is launched.  M3D_EINVAL: a NULL or misaligned pointer, count < 0,
 * an in_size entry < 2, a dim < in_size, start_max < 0 or > dim - size, fixed_origin outside [0, dim - size], need_crop == 0 with dims
 * != in_size, num_boxes < 1, another dtype.  M3D_EUNSUPPORTED: count > 64, num_boxes > 2048, max_boxes < num_boxes, 2^31 candidates or
 * more.  count == 0 does nothing.
 * ------------------------------------------------------------------------------------------------------- */
typedef struct {
  const void* vol; const double* stats; const float* boxes;
  int dtype, depth, height, width, num_boxes;
  int start_max[3];
} m3d_train_image;
int m3d_train_sample(const m3d_train_image* images, int count, const int* in_size, int need_crop, const uint64_t* seeds,
                     const int* fixed_origin, int max_boxes, float* d_data, float* d_boxes, int32_t* d_keep, int32_t* d_info,
                     double* d_score, void* d_ws, size_t* ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Backward of the fully-connected layers (fc_backward.hip; DESIGN, "Box-head backward"): the autograd of nn.Linear at
 * lib/modeling/fast_rcnn_heads.py:84-85,114-117 (fc1, fc2) and :15-19,42-45 (cls_score, bbox_pred), on the operands as PyTorch stores
 * them - no transposed copy of any operand is made.
 *   m3d_linear_dgrad   d_gx [M,K] = d_gy [M,N] . d_weight [N,K]
 *   m3d_linear_wgrad   d_gw [N,K] = d_gy [M,N]^T . d_x [M,K];  d_gb [N] (or NULL) = sum over m of d_gy[m,n], out of the same launch
 * fp32-input MFMA GEMMs (v_mfma_f32_32x32x2_f32), fp32 accumulation.  Where the output has few tiles the reduction is cut into at most
 * 64 slices, a function of (M, N, K) only; the partial sums live in d_ws and are added in slice order, and d_gb is summed in row order
 * without atomics: results are bit-identical run to run.  Error bound per element, with R the reduction length (N for dgrad, M for wgrad
 * and d_gb) and S the slices: |out - out64| <= gamma_n sum |a_k b_k| + 2^-24 |out64|, n = R + S, gamma_n = n 2^-24 / (1 - n 2^-24), the
 * sums taken in fp64 from the fp32 inputs; an output whose products are all zero is exactly 0.
 * d_weight, d_x, d_gx, d_gw: K % 4 == 0 and 16-byte aligned, as m3d_linear_forward.  d_gy: any M, N >= 1 at 4-byte alignment (rows that
 * are not 16-byte multiples are loaded element by element).
 * Limits, checked before any device pointer is followed or anything is launched.  M3D_EINVAL: a NULL required pointer, a pointer that is
 * not 4-byte aligned, N < 1, K < 1, M < 0, d_ws NULL or ws_bytes smaller than the matching *_workspace_bytes (which may be 0: then
 * d_ws may be NULL).  M3D_EUNSUPPORTED: K % 4 != 0, a big operand (or a needed d_ws) that is not 16-byte aligned, an operand of 2^31
 * elements or more.  M == 0: dgrad does nothing; wgrad zero-fills d_gw, and d_gb if given (d_gy and d_x are not looked at).
 * The workspace sizes are multiples of 16 and non-decreasing in M.
 * ------------------------------------------------------------------------------------------------------- */
size_t m3d_linear_dgrad_workspace_bytes(int M, int N, int K);
int m3d_linear_dgrad(const float* d_gy, const float* d_weight, float* d_gx, int M, int N, int K, void* d_ws, size_t ws_bytes,
                     void* stream);
size_t m3d_linear_wgrad_workspace_bytes(int M, int N, int K);
int m3d_linear_wgrad(const float* d_gy, const float* d_x, float* d_gw, float* d_gb, int M, int N, int K, void* d_ws, size_t ws_bytes,
                     void* stream);

/* The same two GEMMs on the f16 matrix cores at fp32 accuracy (fc_backward_f16.hip; DESIGN, "Box-head backward on the f16 pipe"): the
 * "f16x2 split" of m3d_linear_f16x2_forward on the raw fp32 operands - every value is multiplied by its tensor's power of two and cut
 * into two fp16 numbers once, on its way to LDS; three v_mfma_f32_32x32x16_f16 products per fp32 product accumulate in fp32, an
 * accumulator is folded into fp32 registers after at most 384 chained MFMAs.  No packed or transposed copy of any operand is made.
 * d_gb (or NULL) is summed from the uncut fp32 values in a fixed order.  Split reduction, workspace partials added in slice order, no
 * atomics: bit-identical run to run.
 * Bounds: each operand's bound is a device pointer to `slots` floats whose LARGEST is >= the tensor's largest magnitude (1: an
 * m3d_absmax result; m3d_conv3d_zw_slots(): a slot array), or NULL: the call sweeps that operand itself into d_ws (no host read).  A
 * bound smaller than the largest magnitude overflows fp16; a bound up to 2^8 too large costs no accuracy.
 * m3d_linear_backward_f16x2_supported: 1 where M >= 1, N >= 64, N % 4 == 0, K % 4 == 0 and no operand has 2^31 elements or more, else 0
 * (cls_score / bbox_pred stay on m3d_linear_dgrad / m3d_linear_wgrad).
 * The _plan functions (host only) give what the launch runs: slices = the slices of the reduction (1: no second launch), chain = the
 * most MFMAs an accumulator chains (<= 384), folds = the folds of one slice's accumulator into fp32 registers (0: the accumulator is
 * stored directly).  Any output pointer may be NULL.  An output element therefore sees at most chain * max(folds, 1) + folds + slices + 2
 * roundings of its running sum (the last 2: the two scale multiplies) - the n_acc of tests/linear_backward_f16_cases.py.
 * Checked before any pointer is followed, in this order: M < 0, N < 1, K < 1 -> M3D_EINVAL (the plans: M < 1 as well); a shape that
 * _supported refuses -> M3D_EUNSUPPORTED; a NULL required pointer (d_ws is required: the sizes below are never 0 for a supported
 * shape), slots outside 1..1024, a pointer that is not 4-byte aligned, ws_bytes too small -> M3D_EINVAL; an operand, output or d_ws
 * that is not 16-byte aligned -> M3D_EUNSUPPORTED.  M == 0: as m3d_linear_dgrad / m3d_linear_wgrad. */
int m3d_linear_backward_f16x2_supported(int M, int N, int K);
int m3d_linear_dgrad_f16x2_plan(int M, int N, int K, int* slices, int* chain, int* folds);
int m3d_linear_wgrad_f16x2_plan(int M, int N, int K, int* slices, int* chain, int* folds);
size_t m3d_linear_dgrad_f16x2_workspace_bytes(int M, int N, int K);
size_t m3d_linear_wgrad_f16x2_workspace_bytes(int M, int N, int K);
int m3d_linear_dgrad_f16x2(const float* d_gy, const float* d_weight, float* d_gx, int M, int N, int K, const float* d_gy_bound,
                           int gy_bound_slots, const float* d_w_bound, int w_bound_slots, void* d_ws, size_t ws_bytes, void* stream);
int m3d_linear_wgrad_f16x2(const float* d_gy, const float* d_x, float* d_gw, float* d_gb, int M, int N, int K, const float* d_gy_bound,
                           int gy_bound_slots, const float* d_x_bound, int x_bound_slots, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Peak stimulation (peak_stim.hip; DESIGN, "Peak stimulation"): lib/prm/peak_stimulation_3d.py:6-52 on a response map
 * d_x fp32 [B,C,S,H,W], contiguous; win odd, o = win / 2.
 *   peak map     voxel v is a peak iff it is the arg-max of its window [z-o,z+o] x [y-o,y+o] x [x-o,x+o] clipped to the volume; ties go
 *                to the first maximum in raster order (z outer, x inner); a NaN beats everything and among NaNs the last in raster order
 *                wins (what max_pool3d + `indices == element_map` give, :15-25).  -inf is an ordinary, smallest value (the reference's
 *                answer there depends on its -inf padding).  An all-equal volume has one peak per (b,c), at (0,0,0).
 *   filter       filter_kind != NONE: a peak must also satisfy x >= d_thresh[b,c] (false for a NaN on either side, :29).  MEDIAN =
 *                torch.median's lower median (rank (n-1)/2 ascending of the n = S H W values, NaN if the channel holds a NaN, by a radix
 *                select; of -0.0 / +0.0 it returns +0.0); MEAN = the fp64 sum in a fixed order / n, rounded to fp32 once; MAX (NaN if
 *                the channel holds one); CONST = filter_value; TENSOR = d_thresh_in [B*C] as given.  d_thresh [B*C] is always written
 *                (-inf for NONE).
 *   peak list    d_peaks int32 [cap,5] = rows (b,c,z,y,x) in raster order over the whole tensor (torch.nonzero's order, :31); *d_num
 *                (and *h_num, a device-accessible pinned HOST mirror written by the same launch, may be NULL - as
 *                m3d_prm_select_peaks has) = the true count, even above cap; rows beyond cap are not written.  cap may be 0.
 *   aggregation  d_agg [B*C] (may be NULL) = (float)(sum of x * peak over the channel / count) (:38-39): fp64, the 1024-voxel raster
 *                chunks of a channel each summed by a fixed tree and the chunks added in raster order; count == 0 gives NaN; a NaN or
 *                inf voxel that is no peak gives NaN as well (0 * NaN), as in the reference.
 *   d_peak_map   uint8 [B,C,S,H,W] (may be NULL: the map then lives in the workspace): 1 at every peak that passed the filter.
 * Five small launches, no global atomics, no host synchronisation; bit-identical run to run.
 * m3d_peak_stimulation3d_backward (:43-48): d_gx [B,C,S,H,W] = d_peak_map * d_gy[b,c], every element written.
 * Refusals, before any device pointer is followed or anything is launched.  M3D_EINVAL: win even or < 1, an unknown filter_kind, B or
 * C < 0, S, H or W < 1, cap < 0, a NULL required pointer (d_x, d_num, d_thresh, d_ws; d_peaks with cap > 0; d_thresh_in with TENSOR),
 * ws_bytes below m3d_peak_stimulation3d_workspace_bytes.  M3D_EUNSUPPORTED: win > 9, S H W >= 2^31, more tiles or chunks than one grid
 * dimension holds.  B * C == 0: nothing is launched or written.  The workspace size is 0 for arguments the call would refuse.
 * ------------------------------------------------------------------------------------------------------- */
#define M3D_PEAK_FILTER_NONE 0
#define M3D_PEAK_FILTER_MEDIAN 1
#define M3D_PEAK_FILTER_MEAN 2
#define M3D_PEAK_FILTER_MAX 3
#define M3D_PEAK_FILTER_CONST 4
#define M3D_PEAK_FILTER_TENSOR 5
/* peak_stimulation_3d.py:6-52: bytes of d_ws for one m3d_peak_stimulation3d call of these dimensions */
size_t m3d_peak_stimulation3d_workspace_bytes(int B, int C, int S, int H, int W, int win);
/* peak_stimulation_3d.py:6-52 (forward, :8-41) */
int m3d_peak_stimulation3d(const float* d_x, int B, int C, int S, int H, int W, int win, int filter_kind, float filter_value,
                           const float* d_thresh_in, uint8_t* d_peak_map, int32_t* d_peaks, int cap, int64_t* d_num, int64_t* h_num,
                           float* d_thresh, float* d_agg, void* d_ws, size_t ws_bytes, void* stream);
/* peak_stimulation_3d.py:6-52 (backward, :43-48) */
int m3d_peak_stimulation3d_backward(const uint8_t* d_peak_map, const float* d_gy, int B, int C, int S, int H, int W, float* d_gx,
                                    void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * Mask-head up-conv (upconv3d.hip; DESIGN, "Mask-head up-conv"): nn.ConvTranspose3d(kernel 2, stride 2, padding 0) at
 * lib/modeling/mask_rcnn_heads.py:156 with the ReLU of :193, and their autograd.  d_x fp32 [R,Cin,D,H,W], d_weight [Cin,Cout,2,2,2] (the
 * layout of nn.ConvTranspose3d.weight), d_bias [Cout] or NULL, d_y / d_gy / d_y_mask [R,Cout,2D,2H,2W], all contiguous.
 *   m3d_upconv3d_2x_forward  d_y[r,co,2z+a,2y+b,2x+c] = d_bias[co] + sum_ci d_x[r,ci,z,y,x] d_weight[ci,co,a,b,c], then max(., 0) if relu
 *   with g = d_gy where d_y_mask is NULL, else d_gy where d_y_mask > 0 and 0 elsewhere (d_y_mask: the d_y a relu forward wrote):
 *   m3d_upconv3d_2x_dgrad    d_gx[r,ci,z,y,x] = sum over (co,a,b,c) of g[r,co,2z+a,2y+b,2x+c] d_weight[ci,co,a,b,c]
 *   m3d_upconv3d_2x_wgrad    d_gw[ci,co,a,b,c] = sum over (r,z,y,x) of d_x[r,ci,z,y,x] g[r,co,2z+a,2y+b,2x+c];
 *                            d_gb[co] (or NULL) = sum of g[r,co,.,.,.], out of the same launch
 * The outputs never overlap, so each is one fp32-input MFMA GEMM (v_mfma_f32_32x32x2_f32), fp32 accumulation, that addresses the 2x
 * tensor directly: no [R, 8 Cout, D H W] intermediate, no separate bias, ReLU or ReLU-backward pass.  Every element of d_y, d_gx, d_gw
 * and d_gb is written by the call.  Where the output of dgrad / wgrad has few tiles the reduction is cut into at most 64 slices, a
 * function of the shape only; the partial sums live in d_ws and are added in slice order, and d_gb is summed in a fixed order without
 * atomics: results are bit-identical run to run.  Error bound per element, with L the reduction length (Cin forward, 8 Cout dgrad,
 * R D H W wgrad, 8 R D H W for d_gb) and S the partials added (1 where nothing is split; the forward counts its bias instead):
 * |out - out64| <= gamma_n sum |a_k b_k| + 2^-24 |out64|, n = L + S, gamma_n = n 2^-24 / (1 - n 2^-24), the sums taken in fp64 from the
 * fp32 inputs (the forward's include |bias|); a g element with d_y_mask <= 0 contributes exactly nothing.
 * Limits, checked before any device pointer is followed or anything is launched.  M3D_EINVAL: a NULL required pointer (d_x, d_weight,
 * d_y; d_gy, d_gx, d_gw), a pointer that is not 4-byte aligned, Cin, Cout, D, H or W < 1, R < 0, d_ws NULL or ws_bytes smaller than the
 * matching *_workspace_bytes (which may be 0: then d_ws may be NULL).  M3D_EUNSUPPORTED: d_x, d_weight, d_y, d_gy, d_y_mask, d_gx, d_gw
 * or a needed d_ws not 16-byte aligned, an operand of 2^31 elements or more.  R == 0: forward and dgrad do nothing (no pointer is
 * looked at); wgrad zero-fills d_gw, and d_gb if given.  The workspace sizes are multiples of 16 and non-decreasing in R.
 * ------------------------------------------------------------------------------------------------------- */
/* host only: the partial sums S one output element is added up from; kind 0 forward (always 1), 1 dgrad, 2 wgrad; 0: a refused shape */
int m3d_upconv3d_2x_slices(int kind, int R, int Cin, int Cout, int D, int H, int W);
int m3d_upconv3d_2x_forward(const float* d_x, const float* d_weight, const float* d_bias, float* d_y, int R, int Cin, int Cout, int D,
                            int H, int W, int relu, void* stream);
size_t m3d_upconv3d_2x_dgrad_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W);
int m3d_upconv3d_2x_dgrad(const float* d_gy, const float* d_y_mask, const float* d_weight, float* d_gx, int R, int Cin, int Cout, int D,
                          int H, int W, void* d_ws, size_t ws_bytes, void* stream);
size_t m3d_upconv3d_2x_wgrad_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W);
int m3d_upconv3d_2x_wgrad(const float* d_gy, const float* d_y_mask, const float* d_x, float* d_gw, float* d_gb, int R, int Cin, int Cout,
                          int D, int H, int W, void* d_ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The up-conv's FORWARD on the f16 matrix cores at fp32 accuracy, and the mask head's tail in one launch (upconv3d_f16.hip; DESIGN,
 * "Mask-head tail on the f16 pipe").  The f16x2 cut of the ZnConv3d kernels: x and the weight scaled by the power of two of their
 * bounds, cut into hi + lo fp16, three f16 MFMA products per fp32 product, fp32 accumulation, exact un-scaling.  x is cut while it is
 * staged from the fp32 tensor; the weight by the pack call, once: m3d_upconv3d_2x_f16x2_packed_bytes(Cin, Cout) bytes (0: refused)
 * that hold the fragments and, behind them, fl(max|W|) computed on the device (no host read, no atomics).
 *   m3d_upconv3d_2x_forward_f16x2  d_y [R,Cout,2D,2H,2W] as m3d_upconv3d_2x_forward writes it (bias, optional ReLU)
 *   m3d_mask_tail_f16x2            d_out[r,k,2z+a,2y+b,2x+c] = act(d_cls_bias[k] + sum_co d_cls_weight[k,co] max(y[r,co,..], 0)), y the
 *                                  up-conv with d_up_bias; d_cls_weight [K,Cout], 1 <= K <= 8; act = identity (sigmoid 0) or the device
 *                                  sigmoid of m3d_conv3d_forward_split_sigmoid (sigmoid 1: bit-equal to torch.sigmoid of the sigmoid-0
 *                                  output).  The [R,Cout,2D,2H,2W] tensor is never written; no workspace.
 * d_in_max: the [m3d_conv3d_zw_slots()] device floats whose largest bounds max|x| (what the conv before left, or
 * m3d_conv3d_zw_bound_of).  No atomics, every output element written by the call, bit-identical run to run, no scratch; an Inf / NaN
 * operand gives NaN, never a finite number.  Error bounds per element: tests/upconv_f16_cases.py (c1 = 3.01, n_acc = 3 Cin / 16,
 * m = Cout + 2).
 * m3d_upconv3d_2x_f16x2_supported (host only): Cin % 16 == 0, Cout, D, H, W >= 1, R >= 0, and x, y and the padded pack below 2^31
 * elements.  Refusals, all before a pointer is followed: M3D_EINVAL for R < 0 or Cin, Cout, D, H or W < 1, a NULL required pointer, a
 * pointer that is not 4-byte aligned; M3D_EUNSUPPORTED for a shape _supported refuses, K outside 1..8, the tail's output of 2^31
 * elements or more, d_packed not 16-byte or the output not 8-byte aligned.  R == 0 does nothing (no pointer is looked at).
 * ------------------------------------------------------------------------------------------------------- */
int m3d_upconv3d_2x_f16x2_supported(int R, int Cin, int Cout, int D, int H, int W);
size_t m3d_upconv3d_2x_f16x2_packed_bytes(int Cin, int Cout);
int m3d_upconv3d_2x_f16x2_pack(const float* d_weight, int Cin, int Cout, void* d_packed, void* stream);
int m3d_upconv3d_2x_forward_f16x2(const float* d_x, const void* d_packed, const float* d_bias, float* d_y, int R, int Cin, int Cout, int D,
                                  int H, int W, int relu, const float* d_in_max, void* stream);
int m3d_mask_tail_f16x2(const float* d_x, const void* d_packed, const float* d_up_bias, const float* d_cls_weight, const float* d_cls_bias,
                        float* d_out, int R, int Cin, int Cout, int K, int D, int H, int W, int sigmoid, const float* d_in_max,
                        void* stream);

/* ---------------------------------------------------------------------------------------------------------
 * The up-conv's BACKWARD on the f16 matrix cores at fp32 accuracy (upconv3d_bwd_f16.hip; DESIGN, "Up-conv backward on the f16 pipe"):
 * what m3d_upconv3d_2x_dgrad / _wgrad compute, on the same tensors as PyTorch stores them (d_gy, d_y_mask [R,Cout,2D,2H,2W], d_x
 * [R,Cin,D,H,W], d_weight [Cin,Cout,2,2,2]; no transposed, shuffled or packed copy of any of them).  With g = d_gy where d_y_mask > 0
 * (d_y_mask NULL: g = d_gy; a select applied before the cut, so a masked-out Inf / NaN contributes exactly 0), n = 8 co + 4a + 2b + c
 * and col = (r, z, y, x):
 *   m3d_upconv3d_2x_dgrad_f16x2   d_gx[col, ci] = sum_n g[col, n] W[ci, n]                       (reduction 8 Cout, never split)
 *   m3d_upconv3d_2x_wgrad_f16x2   d_gw[ci, n] = sum_col x[col, ci] g[col, n]                     (reduction R D H W, split-K into d_ws)
 *                                 d_gb[co] (or NULL) = sum g, from the UNCUT fp32 values in a fixed order, out of the same launch
 * The f16x2 cut of f16x2.h: each operand times the power of two of its tensor bound, cut into hi + lo fp16 once while it is staged,
 * three v_mfma_f32_32x32x16_f16 per fp32 product, fp32 accumulation, exact un-scaling.  d_gy_max / d_w_max / d_x_max: the
 * [m3d_conv3d_zw_slots()] device floats whose largest bounds the operand (for g: the UNMASKED d_gy), or NULL: the call sweeps that
 * operand into d_ws (no host read).  d_ws: _workspace_bytes(...) bytes (0: the shape is refused), 16-byte aligned; every byte of it
 * the call reads it has written.  No atomics, every output element written by the call, bit-identical run to run and on any stream,
 * no scratch; an Inf / NaN in an unmasked operand gives NaN, never a finite number.
 * Error bounds per element: tests/upconv_backward_f16_cases.py - the formula of tests/f16x2_contract.py with c1 = 3.01 (no operand is
 * rounded before the cut) and n_acc = chain * max(folds, 1) + folds + slices + 2 from the _plan calls (host only): `slices` partial
 * sums the reduce launch adds (dgrad: always 1), `chain` the most MFMAs one accumulator chains between two fp32 folds (<= 384), `folds`
 * the folds of a slice (0: the chain is never folded); + 2: the two scale multiplies.  d_gb: the fp32 bound of upconv_reference.bound
 * with n = 8 R D H W + gb_partials.
 * m3d_upconv3d_2x_backward_f16x2_supported (host only): R, D, H, W >= 1, Cin % 32 == 0, Cout % 32 == 0, every tensor below 2^31
 * elements.  Refusals, all before a pointer is followed: M3D_EINVAL for R < 0 or Cin, Cout, D, H or W < 1, a NULL required pointer
 * (d_ws included), a pointer that is not 4-byte aligned, a workspace that is too small; M3D_EUNSUPPORTED for a shape _supported
 * refuses and for d_gy, d_y_mask, d_weight, d_gw or d_ws not 16-byte aligned.  R == 0: dgrad does nothing (no pointer is looked at),
 * wgrad writes zeros to d_gw and d_gb.
 * ------------------------------------------------------------------------------------------------------- */
int m3d_upconv3d_2x_backward_f16x2_supported(int R, int Cin, int Cout, int D, int H, int W);
int m3d_upconv3d_2x_dgrad_f16x2_plan(int R, int Cin, int Cout, int D, int H, int W, int* slices, int* chain, int* folds);
int m3d_upconv3d_2x_wgrad_f16x2_plan(int R, int Cin, int Cout, int D, int H, int W, int* slices, int* chain, int* folds, int* gb_partials);
size_t m3d_upconv3d_2x_dgrad_f16x2_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W);
size_t m3d_upconv3d_2x_wgrad_f16x2_workspace_bytes(int R, int Cin, int Cout, int D, int H, int W);
int m3d_upconv3d_2x_dgrad_f16x2(const float* d_gy, const float* d_y_mask, const float* d_weight, float* d_gx, int R, int Cin, int Cout,
                                int D, int H, int W, const float* d_gy_max, const float* d_w_max, void* d_ws, size_t ws_bytes,
                                void* stream);
int m3d_upconv3d_2x_wgrad_f16x2(const float* d_gy, const float* d_y_mask, const float* d_x, float* d_gw, float* d_gb, int R, int Cin,
                                int Cout, int D, int H, int W, const float* d_gy_max, const float* d_x_max, void* d_ws, size_t ws_bytes,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M3D_H_ */
