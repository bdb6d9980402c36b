/*
 * upsnet_hip.h -- C ABI of libupsnet_hip.so: the MI355X (gfx950 / CDNA4) replacement for the native
 * operators on UPSNet's per-image inference hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - Alignment: every device pointer is 16-byte aligned. The kernels use 128-bit loads and stores, 64-bit atomics on parts carved from
 *     byte workspaces at 16-byte steps, and 4-byte fills; none of the entry points checks the address (the Python binding does, before
 *     the call: upsnet_amd/_lib.py). Exempt, element alignment suffices: mask_logit of upsnet_mask_logit_gather; the maps behind
 *     cls_prob[] and bbox_pred[] of upsnet_pyramid_proposals_strided / _strided_ordered / _joint_strided; sseg and pano of
 *     upsnet_restore_label_maps; src of upsnet_restore_plane_u8. Their kernels read one element per access at a caller-given stride.
 *     Host pointers only feed copies or launch arithmetic and are outside the rule;
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream; NULL = default stream);
 *   - the caller allocates every output and every workspace (the reference does the same:
 *     functions/deform_conv.py:44-45, functions/roialign.py:37); the library never allocates
 *     device memory, except upsnet_nms_host (the `_nms` drop-in, which the reference also lets malloc);
 *   - functions return 0 on success, non-zero on error; upsnet_last_error() then describes it
 *     (the reference returned 1/0 and printed, SURVEY.md section 8b "Errors");
 *   - layouts: "nchw" entry points take the reference's contiguous NCHW tensors and are drop-in
 *     replacements for the reference natives; "nhwc" entry points are the MI355X-native fast path
 *     (channels-last physical layout so that a bilinear tap is one contiguous C-vector).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the reference
 * repository root, uber-research/UPSNet).
 */
#ifndef UPSNET_HIP_H
#define UPSNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Last error message of the calling thread ("" if none). */
const char *upsnet_last_error(void);
/* Name of the kernel instance the calling thread's most recent convolution launch took where the choice is made inside the library
 * (bf16-mode convolutions: "conv3x3_wreg<8,2>", "conv1x1_wreg<4,1>", "conv3x3_halo", "conv_bf16<2>"; Winograd: "wino<0,64,128>").
 * Test introspection (tests/test_layerwise_gpu.py asserts the forms a benchmarked configuration runs on); "" before any launch. */
const char *upsnet_last_kernel_form(void);
/* Library ABI version (bumped on any signature change). */
int upsnet_abi_version(void);

/* Zero `bytes` bytes at `ptr` (any alignment) with a plain kernel on `stream`. The scratch of the selection ops is cleared this way
 * instead of hipMemsetAsync (a replacement for the reference's THCudaTensor zero_() / cudaMemset of its scratch, e.g.
 * upsnet/nms/nms_kernel.cu:112-113): a captured forward then holds kernel nodes only (memset nodes fault at graph replay). */
int upsnet_zero_fill(void *stream, void *ptr, size_t bytes);

/* ============================== ROIAlign ============================== */

/* Replaces roi_align_forward_gpu_kernel_launcher (upsnet/operators/src/roi_align_cuda.cpp:26-30,
 * bound to Python as roi_align_cuda.roi_align_forward, roi_align_cuda.cpp:39-75,114-118).
 * bottom_data [B,C,H,W] NCHW, bottom_rois [N,5] = (batch,x1,y1,x2,y2), top_data [N,C,PH,PW]. */
int upsnet_roi_align_forward(void *stream, const float *bottom_data, float spatial_scale, int num_rois,
                             int height, int width, int channels, int pooled_height, int pooled_width,
                             int sampling_ratio, const float *bottom_rois, float *top_data);

/* Same op on channels-last features: feat [B,H,W,C], out [N,PH,PW,C]. C % 4 == 0. */
int upsnet_roi_align_forward_nhwc(void *stream, const float *feat_nhwc, int batch, int height, int width,
                                  int channels, float spatial_scale, const float *rois, int num_rois,
                                  int pooled_height, int pooled_width, int sampling_ratio, float *out_nhwc);

/* Replaces FPNRoIAlign.forward (upsnet/operators/modules/fpn_roi_align.py:32-62): level assignment
 * floor(2+log2(sqrt(wh)/224+1e-6)) on device, all four levels in one launch, output in the
 * original ROI order. feat_nhwc[l] is [H_l,W_l,C]; out_nhwc [N,PH,PW,C]; levels_out (optional) [N].
 * num_rois_dev (optional): device int32 with the number of valid rois (<= num_rois); rows beyond it
 * are written as zeros. The pointer arrays themselves are HOST arrays of 4 entries. */
int upsnet_fpn_roi_align_forward(void *stream, const float *const feat_nhwc[4], const int feat_h[4],
                                 const int feat_w[4], const float spatial_scale[4], int channels,
                                 const float *rois, int num_rois, const int *num_rois_dev, int pooled_height,
                                 int pooled_width, int sampling_ratio, float *out_nhwc, int *levels_out);

/* r13: the same launch with a workgroup -> ROI table: workgroup b takes ROI order[b] (order == NULL: its own index). Output rows stay at the
 * ROI's own index: results are bit-identical whatever the table, only the workgroup -> XCD assignment changes (workgroup b runs on XCD
 * b % 8, each XCD has its own L2). upsnet_fpn_roi_order fills the table so that every XCD's workgroups take one contiguous range of the
 * ROIs bucketed by (pyramid level, 1/16 stripe of the image, 1/8 column cell; image_height x image_width = the extent the ROIs live in):
 * neighbouring ROIs share an L2 instead of every L2 fetching its own
 * copy of the shared pyramid cells (FPNRoIAlign.forward, upsnet/operators/modules/fpn_roi_align.py:32-62, processes level by level too).
 * num_rois <= 2048 for the table; caller-allocated int[num_rois]. The table is a permutation of 0..num_rois-1 and each bucket's range
 * of positions is fixed, but the order of the ROIs inside one bucket is unspecified (slots are taken with atomics). */
int upsnet_fpn_roi_order(void *stream, const float *rois, int num_rois, const int *num_rois_dev, int image_height, int image_width,
                         int *order_out);
int upsnet_fpn_roi_align_forward_ordered(void *stream, const float *const feat_nhwc[4], const int feat_h[4], const int feat_w[4],
                                         const float spatial_scale[4], int channels, const float *rois, int num_rois, const int *num_rois_dev,
                                         int pooled_height, int pooled_width, int sampling_ratio, float *out_nhwc, int *levels_out,
                                         const int *order);

/* Development knob of upsnet_fpn_roi_align_forward: 0 = LDS tap-table kernel, one register set; 1 = two sets;
 * 2 = the r03-r07 kernel (per-bin tap setup in registers); 3 = the table kernel loading only the UNIQUE corner cells of a bin (r11);
 * 4 = 3 with packed fp32 blend arithmetic; < 0 = back to the default behaviour: the environment variable UPSNET_ROI_KERNEL (a variant number)
 * if set, else automatic -- 3 for launches with >= 100 bins per ROI, else 0. A call with variant >= 0 overrides the variable. All variants
 * return the same bits. upsnet_roi_geometry: the bins of a ROI are split over
 * workgroups until the launch has `target_workgroups` (default 1536), at least `min_bins` (default 8) bins each; 0 = default. */
void upsnet_roi_tuning(int variant);
void upsnet_roi_geometry(int target_workgroups, int min_bins);

/* ============================== Deformable convolution ============================== */

/* Replaces deformable_im2col_gpu_kernel_launcher (upsnet/operators/src/deform_conv_cuda.cpp:25-30,
 * bound as deform_conv_cuda.deform_im2col, deform_conv_cuda.cpp:49-68). NCHW, parallel_imgs images.
 * data_col is [C*kh*kw, parallel_imgs, Ho, Wo]. */
int upsnet_deform_im2col(void *stream, const float *data_im, const float *data_offset, int channels,
                         int height, int width, int ksize_h, int ksize_w, int pad_h, int pad_w, int stride_h,
                         int stride_w, int dilation_h, int dilation_w, int parallel_imgs, int deformable_group,
                         float *data_col);

/* Replaces modulated_deformable_im2col_gpu_kernel_launcher
 * (upsnet/operators/src/mod_deform_conv_cuda.cpp:24-31, bound as mod_deform_im2col :51-74). */
int upsnet_mod_deform_im2col(void *stream, const float *data_im, const float *data_offset,
                             const float *data_mask, int batch_size, int channels, int height_im, int width_im,
                             int height_col, int width_col, int kernel_h, int kernel_w, int pad_h, int pad_w,
                             int stride_h, int stride_w, int dilation_h, int dilation_w, int deformable_group,
                             float *data_col);

/* ---- backward natives of the same pybind modules (API parity for fine-tuning; not on the inference path).
 * fp32 NCHW, argument order of the reference launchers. The scatter kernels accumulate INTO their output with
 * fp32 atomics exactly like the reference (zero it first; summation order unspecified => parity 1e-5-level);
 * the col2im_coord gathers have a fixed order and are bit-exact against the oracle. */

/* Replaces roi_align_backward_gpu_kernel_launcher (upsnet/operators/src/roi_align_cuda.cpp:32-36, bound as
 * roi_align_cuda.roi_align_backward :77-112; kernel roi_align_kernel.cu:238-349). top_diff [N,C,PH,PW],
 * bottom_diff [B,C,H,W] accumulated. */
int upsnet_roi_align_backward(void *stream, const float *top_diff, float spatial_scale, int batch_size, int num_rois,
                              int height, int width, int channels, int pooled_height, int pooled_width,
                              int sampling_ratio, const float *bottom_rois, float *bottom_diff);

/* Replaces deformable_col2im_gpu_kernel_launcher (deform_conv_cuda.cpp:32-38, bound as deform_col2im :70-86;
 * kernel deform_conv_kernel.cu:293-383). data_col [C*kh*kw, parallel_imgs, Ho, Wo] -> grad_im accumulated. */
int upsnet_deform_col2im(void *stream, const float *data_col, const float *data_offset, int channels, int height,
                         int width, int ksize_h, int ksize_w, int pad_h, int pad_w, int stride_h, int stride_w,
                         int dilation_h, int dilation_w, int parallel_imgs, int deformable_group, float *grad_im);

/* Replaces deformable_col2im_coord_gpu_kernel_launcher (deform_conv_cuda.cpp:40-46, bound as deform_col2im_coord
 * :88-105; kernel deform_conv_kernel.cu:391-500). grad_offset is overwritten. */
int upsnet_deform_col2im_coord(void *stream, const float *data_col, const float *data_im, const float *data_offset,
                               int channels, int height, int width, int ksize_h, int ksize_w, int pad_h, int pad_w,
                               int stride_h, int stride_w, int dilation_h, int dilation_w, int parallel_imgs,
                               int deformable_group, float *grad_offset);

/* Replaces modulated_deformable_col2im_gpu_kernel_launcher (mod_deform_conv_cuda.cpp:33-40, bound as
 * mod_deform_col2im :76-92; kernel mod_deform_conv_kernel.cu:251-311, launcher :409-433). Like the reference
 * launcher (:423) the kernel receives pad_h for BOTH paddings; pad_w is accepted and ignored. */
int upsnet_mod_deform_col2im(void *stream, const float *data_col, const float *data_offset, const float *data_mask,
                             int batch_size, int channels, int height_im, int width_im, int height_col, int width_col,
                             int kernel_h, int kernel_w, int pad_h, int pad_w, int stride_h, int stride_w,
                             int dilation_h, int dilation_w, int deformable_group, float *grad_im);

/* Replaces modulated_deformable_col2im_coord_gpu_kernel_launcher (mod_deform_conv_cuda.cpp:42-50, bound as
 * mod_deform_col2im_coord :94-114; kernel mod_deform_conv_kernel.cu:313-381). grad_offset / grad_mask overwritten. */
int upsnet_mod_deform_col2im_coord(void *stream, const float *data_col, const float *data_im, const float *data_offset,
                                   const float *data_mask, int batch_size, int channels, int height_im, int width_im,
                                   int height_col, int width_col, int kernel_h, int kernel_w, int pad_h, int pad_w,
                                   int stride_h, int stride_w, int dilation_h, int dilation_w, int deformable_group,
                                   float *grad_offset, float *grad_mask);

/* Fused deformable convolution forward (v1 when mask == NULL, v2 otherwise), the MI355X-native
 * replacement for DeformConvFunction.forward's im2col + torch.mm (functions/deform_conv.py:43-57)
 * with no column buffer: the dense implicit-GEMM kernel below with a bilinear-gather A operand
 * (fp32 MFMA, v_mfma_f32_32x32x2_f32). Up to 4 feature maps that share the same weights (the FCN
 * head's four FPN levels) go in ONE launch.
 *   x[l]      [H_l, W_l, Cin]  NHWC (batch 1)
 *   offset[l] [Ho_l, Wo_l, 2*kh*kw] NHWC (channel order as the reference: 2*(i*kw+j) = dh, +1 = dw)
 *   mask[l]   [Ho_l, Wo_l, kh*kw]  NHWC, or mask == NULL
 *   wpack     [kh*kw*Cin, ldw] from upsnet_conv_pack_weight; bias [Cout] or NULL
 *   out[l]    [Ho_l, Wo_l, Cout] NHWC;  relu != 0 fuses max(.,0).
 * Pointer/shape arrays are HOST arrays of nlev entries. Cin % 32 == 0, deformable_group == 1. */
int upsnet_deform_conv_forward_nhwc(void *stream, int nlev, const float *const x[], const float *const offset[],
                                    const float *const mask[], float *const out[], const int height[],
                                    const int width[], int cin, int cout, int kh, int kw, int pad_h, int pad_w,
                                    int stride_h, int stride_w, int dil_h, int dil_w, int deformable_group,
                                    const float *wpack, int ldw, const float *bias, int relu);

/* Second-generation fused deformable convolution (csrc/deform_fused.hip): same operator and tensor layouts as
 * upsnet_deform_conv_forward_nhwc (replaces DeformConvFunction.forward, functions/deform_conv.py:43-57, and the modulated
 * v2 form, mod_deform_conv_kernel.cu:187-249), but the K walk is channel-slab outermost / tap innermost (neighbouring taps
 * re-use their corner lines out of L1 / L2), the per-(pixel, tap) sampling descriptors live in an LDS table built once per
 * workgroup, and the weights are read in MFMA fragment order straight from L2:
 *   wpack: upsnet_dcn_packed_weight_floats(cout, cin, kh, kw) floats, filled by upsnet_dcn_pack_weight from the
 *          nn.Conv2d-layout weight [Cout, Cin, kh, kw]; square pad / stride / dilation; at most 25 taps; Cin % 32 == 0.
 * upsnet_dcn_tuning: development knob (register-set / occupancy variants for A/B runs). */
size_t upsnet_dcn_packed_weight_floats(int cout, int cin, int kh, int kw);
int upsnet_dcn_pack_weight(void *stream, const float *weight, int cout, int cin, int kh, int kw, float *wpack);
int upsnet_deform_conv_fused_nhwc(void *stream, int nlev, const float *const x[], const float *const offset[],
                                  const float *const mask[], float *const out[], const int height[], const int width[],
                                  int cin, int cout, int kh, int kw, int pad, int stride, int dil, const float *wpack,
                                  const float *bias, int relu);
/* Split-K form for ONE small map (the DCN bottlenecks of a ResNet-101-DCN backbone have 96-273 tiles for 256 CUs): the (channel slab,
 * tap) walk is divided over ksplit (2..8) workgroups per tile, raw partial sums go to `workspace`
 * (upsnet_deform_conv_fused_splitk_workspace_bytes) and a fixed-order reduce kernel adds bias / ReLU (deterministic). Cout % 4 == 0. */
size_t upsnet_deform_conv_fused_splitk_workspace_bytes(int height, int width, int cout, int kh, int kw, int pad, int stride, int dil,
                                                       int ksplit);
int upsnet_deform_conv_fused_nhwc_splitk(void *stream, const float *x, const float *offset, const float *mask, float *out, int height,
                                         int width, int cin, int cout, int kh, int kw, int pad, int stride, int dil,
                                         const float *wpack, const float *bias, int relu, int ksplit, void *workspace);
void upsnet_dcn_tuning(int variant);

/* The same fused deformable convolution on the bf16 matrix cores (csrc/deform_fused_bf16.hip; BASELINE.json configs[2], opt-in with
 * the other bf16 kernels): blended samples and weights rounded to bf16 (nearest even), exact products, fp32 accumulation. Arguments
 * as upsnet_deform_conv_fused_nhwc; wpack: upsnet_dcn_pack_weight_bf16 into upsnet_dcn_packed_weight_bf16_elems 2-byte elements. */
size_t upsnet_dcn_packed_weight_bf16_elems(int cout, int cin, int kh, int kw);
int upsnet_dcn_pack_weight_bf16(void *stream, const float *weight, int cout, int cin, int kh, int kw, void *wpack);
int upsnet_deform_conv_fused_nhwc_bf16(void *stream, int nlev, const float *const x[], const float *const offset[],
                                       const float *const mask[], float *const out[], const int height[], const int width[], int cin,
                                       int cout, int kh, int kw, int pad, int stride, int dil, const void *wpack, const float *bias,
                                       int relu);

/* ============================== Input blob (the step before the path) ============================== */

/* BaseDataset.prep_im_for_blob + im_list_to_blob (upsnet/dataset/base_dataset.py:143-173,898-923) in one kernel:
 * image_hwc uint8 [height,width,3] (BGR) -> float32, minus pixel_means (in double, like numpy's float32 -= float64),
 * bilinear resize by im_scale (cv2.resize INTER_LINEAR semantics; identity for im_scale == 1), zero padded to
 * [padded_h, padded_w]. resized_h/w = cvRound(height*im_scale) etc. are computed by the caller (host mirror:
 * upsnet_amd/dataset/blob.py). nhwc4 == 0: blob is planar [3,padded_h,padded_w] (the reference's layout);
 * nhwc4 != 0: blob is [padded_h,padded_w,4] with a zero 4th channel (input of upsnet_conv2d_stem_nhwc4_f32). */
int upsnet_prep_image_u8(void *stream, const unsigned char *image_hwc, int height, int width, const double pixel_means[3],
                         double im_scale, int resized_h, int resized_w, int padded_h, int padded_w, int nhwc4, float *blob);

/* Layout plumbing: fp32 [N,C<=4,H,W] planar -> [N,H,W,4] (missing channels zero). */
int upsnet_image_to_nhwc4(void *stream, const float *nchw, int batch, int channels, int height, int width, float *nhwc4);

/* ============================== Dense convolution ============================== */

/* upsnet_conv2d_nhwc_f32 (below) with per-map weights: wpack[i] packs the weights of map i (same geometry, Cin, Cout, ldw); no bias,
 * no residual. Replaces the four per-level products W_l y_l of the FCN head's 1x1 score layer (upsnet/models/fcn.py:101-104, the
 * 512-channel concat + conv commuted below the bilinear upsamples) as one launch. */
int upsnet_conv2d_nhwc_f32_multiw(void *stream, int nseg, const float *const x[], float *const out[], const int batch[],
                                  const int height[], const int width[], int Cin, const float *const wpack[], int ldw, int Cout,
                                  int KH, int KW, int stride, int pad, int relu);

/* Replaces nn.Conv2d (+ folded frozen BatchNorm + bias + residual add + ReLU) of the backbone / FPN / RPN / heads
 * (upsnet/models/resnet.py:53-100, fpn.py:78-104, rpn.py:52-57, rcnn.py:79-87, fcn.py:88-108): NHWC fp32 implicit
 * GEMM on v_mfma_f32_32x32x2_f32 with a fused epilogue. Up to 5 feature maps sharing the weights per launch.
 *   x[i] [N_i,H_i,W_i,Cin] NHWC (Cin % 32 == 0), wpack [KH*KW*Cin, ldw] from upsnet_conv_pack_weight (ldw = Cout
 *   rounded up to a multiple of 32), bias [Cout] or NULL, residual (NULL or array; entries [N_i,Ho,Wo,Cout]),
 *   out[i] [N_i,Ho,Wo,Cout]; batch == NULL means N_i = 1. Pointer/shape arrays are HOST arrays of nseg entries.
 *   residual_up != 0: residual entries are [N_i,Ho/2,Wo/2,Cout] and are added through a nearest x2 upsampling
 *   (the FPN top-down add, F.interpolate(scale_factor=2, mode='nearest') + sum, fpn.py:34,90-96). */
int upsnet_conv2d_nhwc_f32(void *stream, int nseg, const float *const x[], const float *const residual[],
                           float *const out[], const int batch[], const int height[], const int width[], int Cin,
                           const float *wpack, int ldw, const float *bias, int Cout, int KH, int KW, int stride, int pad,
                           int relu, int residual_up);

/* upsnet_conv2d_nhwc_f32 for ONE small feature map (res4 / res5: 2048-8192 pixels = too few 64x64 tiles to fill 256 CUs): the
 * K walk is split over ksplit (2..8) workgroups per tile, raw partial sums go to `workspace`
 * (upsnet_conv2d_splitk_workspace_bytes) and a second kernel adds them in a fixed order with the bias / residual / ReLU
 * epilogue -- deterministic, differs from the unsplit kernel only by fp32 summation order. */
size_t upsnet_conv2d_splitk_workspace_bytes(int batch, int height, int width, int Cout, int KH, int KW, int stride, int pad, int ksplit);
int upsnet_conv2d_nhwc_f32_splitk(void *stream, const float *x, const float *residual, float *out, int batch, int height, int width,
                                  int Cin, const float *wpack, int ldw, const float *bias, int Cout, int KH, int KW, int stride,
                                  int pad, int relu, int ksplit, void *workspace);

/* 3x3 / stride 1 / pad 1 convolution as Winograd F(2x2, 3x3) on the fp32 MFMA (csrc/conv_wino.hip; 16/36 of the multiplies
 * of the direct form; all arithmetic fp32; differs from the direct kernel by fp32 rounding only, ~1e-5 absolute on unit-scale
 * data -- cuDNN, the reference's convolution backend, uses the same algorithm). Replaces the 3x3 nn.Conv2d layers of
 * upsnet/models/resnet.py:64-77, fpn.py:60-98, rpn.py:34-47 and the mask head rcnn.py:96-116 where the map has enough 2x2
 * tiles. A workgroup keeps all 16 transform-domain accumulators of its 64 tiles x 64 channels in registers: one walk over the
 * input channels, each patch pixel loaded and transformed once, lane-local output transform. Cin % 16 == 0 (conv_fill: % 32),
 * ldw = Cout rounded up to 64; wpack (16 * Cin * ldw floats, fragment order) from upsnet_conv_pack_weight_winograd
 * (weight [Cout,Cin,3,3]). Same calling convention as upsnet_conv2d_nhwc_f32 (multi-map launch, bias / residual / ReLU). */
int upsnet_conv2d_winograd_nhwc_f32(void *stream, int nseg, const float *const x[], const float *const residual[],
                                    float *const out[], const int batch[], const int height[], const int width[], int Cin,
                                    const float *wpack, int ldw, const float *bias, int Cout, int relu);

/* The same convolution of ONE map with the K walk split `ksplit` (2..8) ways -- maps with too few 2x2 tiles to fill 256 CUs
 * (res4 / res5 3x3, FPN P4; replaces the same nn.Conv2d call sites). workspace: upsnet_conv2d_splitk_workspace_bytes(batch,
 * height, width, Cout, 3, 3, 1, 1, ksplit) bytes. Fixed summation order: bit-repeatable. */
int upsnet_conv2d_winograd_nhwc_f32_splitk(void *stream, const float *x, const float *residual, float *out, int batch, int height,
                                           int width, int Cin, const float *wpack, int ldw, const float *bias, int Cout, int relu,
                                           int ksplit, void *workspace);
int upsnet_conv_pack_weight_winograd(void *stream, const float *weight, int cout, int cin, int ldw, float *wpack);

/* The Winograd convolution on 32-tile x 32-CHANNEL workgroups for any Cout (ldw = Cout rounded up to 32; weights packed by
 * upsnet_conv_pack_weight_winograd_tn32): twice the workgroups of the 32 x 64 form with half the work each, bit-identical results --
 * for the part of a launch that would otherwise run as a nearly empty last round (the tail ROIs of the mask head, rcnn.py:96-116). */
int upsnet_conv2d_winograd_nhwc_f32_tn32(void *stream, int nseg, const float *const x[], const float *const residual[],
                                         float *const out[], const int batch[], const int height[], const int width[], int Cin,
                                         const float *wpack, int ldw, const float *bias, int Cout, int relu);
int upsnet_conv_pack_weight_winograd_tn32(void *stream, const float *weight, int cout, int cin, int ldw, float *wpack);
/* One launch of both forms over a batch x [batch, H, W, Cin] (the mask head's 100 ROIs: 616 workgroups of the 32 x 64 form for 512 slots):
 * images [0, n_main) on 32 x 64 workgroups (wpack / ldw), images [n_main, batch) on 32 x 32 workgroups (wpack32 / ldw32), which the
 * dispatcher deals out as the main workgroups retire. out [batch, H, W, Cout]; bit-identical to upsnet_conv2d_winograd_nhwc_f32. */
int upsnet_conv2d_winograd_nhwc_f32_tail(void *stream, const float *x, float *out, int batch, int n_main, int height, int width, int Cin,
                                         const float *wpack, int ldw, const float *wpack32, int ldw32, const float *bias, int Cout, int relu);

/* Dense convolution on the bf16 matrix cores (v_mfma_f32_32x32x16_bf16, fp32 accumulation) -- BASELINE.json configs[2]
 * ("bf16 compute / fp32 accumulate") and its fp32-equivalent 3-term split. OPT-IN: the fp32 kernel above is the default.
 * Activations stay fp32 NHWC in HBM (same tensors as upsnet_conv2d_nhwc_f32) and are split to bf16 on the way into LDS.
 *   wpack_lo == NULL : "bf16"   -- operands rounded to bf16, one MFMA per product
 *   wpack_lo != NULL : "bf16x3" -- a = a_hi + a_lo, b = b_hi + b_lo; a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi (error ~2^-16
 *                      relative per product, fp32 accumulation): inside the 1e-4 fp32-logit tolerance
 * wpack_hi / wpack_lo: bf16 [KH*KW*Cin/32][ldw][32] from upsnet_conv_pack_weight_bf16, ldw = Cout rounded up to 64.
 * Same calling convention as upsnet_conv2d_nhwc_f32 (without residual_up). relu: bit 0 = ReLU; bit 1 = `residual` is at half
 * resolution and is added through a nearest x2 upsampling (1x1 kernels only: the FPN top-down add); bits 2 / 3 / 4 = the input / the
 * output / the residual tensors are bf16 (NHWC, same shapes) instead of fp32 (bf16 mode only, wpack_lo == NULL): hence void. */
int upsnet_conv2d_nhwc_bf16(void *stream, int nseg, const void *const x[], const void *const residual[], void *const out[],
                            const int batch[], const int height[], const int width[], int Cin, const void *wpack_hi,
                            const void *wpack_lo, int ldw, const float *bias, int Cout, int KH, int KW, int stride, int pad,
                            int relu);
int upsnet_conv_pack_weight_bf16(void *stream, const float *weight, int cout, int cin, int kh, int kw, int ldw, void *wpack_hi,
                                 void *wpack_lo);
/* The FIRST bottleneck of a stage (projection shortcut; upsnet/models/resnet.py:84-100) as ONE launch on the bf16 matrix cores:
 *   out = relu(conv3(relu(conv2(relu(conv1_s(x))))) + proj_s(x)),  conv1_s / proj_s: 1x1 with stride s (1 or 2), conv2: 3x3 / 1 / 1.
 * x [N,Hin,Win,Cin] bf16, out [N,H,W,4 Cm] bf16, H = (Hin - 1) / s + 1; (Cm, Cin) in {(64, 64), (128, 256), (256, 512)}. w1: fragments
 * of [Cm, Cin]; w2: of [Cm, 9 Cm] (tap-major k); w3d: of [4 Cm, Cm + Cin] = [W3 | Wd] -- conv3 and the projection are one GEMM over
 * K = [t2 ; x], the shortcut is accumulated in fp32; b1, b2 [Cm]; b3d = b3 + bd [4 Cm]. Fragment order as upsnet_bottleneck_bf16. */
int upsnet_bottleneck_proj_bf16(void *stream, const void *x, void *out, int batch, int height_in, int width_in, int cin, int cmid, int stride,
                                const void *w1, const void *w2, const void *w3d, const float *b1, const float *b2, const float *b3d);
/* A/B switch of the 3x3 / stride 1 / 256 -> 256 layers in the plain bf16 mode (csrc/conv3x3_wreg_bf16.hip: weights fed to the MFMA
 * from L2, one barrier per 32-channel slab): enable 0 = the general haloed-patch kernel, 1 = default; tile_rows 0 = automatic,
 * 8 / 16 = forced tile height, 2 = 2-row tiles (256-channel workgroups), 1 = 2-row tiles with 128-channel workgroups. Same products
 * and K order either way. */
int upsnet_conv_bf16_tuning(int enable, int tile_rows);
/* A/B switch of the 1x1 layers with bf16 activations in the plain bf16 mode (csrc/conv1x1_wreg_bf16.hip: both MFMA operands loaded
 * from global memory in fragment order, no LDS, no barrier): enable 0 = conv_bf16_kernel, 1 = default (the layers it is faster on:
 * shortcut epilogue, Cin <= 256), 2 = every layer it can compute. Same products and K order. */
int upsnet_conv1x1_bf16_tuning(int enable);
/* The backbone stem in one launch on the fp32 matrix cores (upsnet/models/resnet.py:347-356; the headline path): convolution 7x7 /
 * stride 2 / pad 3 (Cin <= 3 -> 64, frozen BN folded: + bias) + ReLU + max-pool 3x3 / stride 2 / pad 1 -- the 134 MB convolution output
 * of a 1024x2048 image never reaches HBM. x4 [N,H,W,4] fp32 (RGB + a zero channel), wpack = upsnet_stem_pool_pack_weight_f32(weight
 * [64,Cin,7,7]) (2 x 75 x 64 floats), bias [64] or NULL, out [N,Hp,Wp,64] fp32, Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1 (likewise the
 * width). Exact fp32 products (v_mfma_f32_32x32x2_f32), fixed summation order. */
int upsnet_stem_pool_pack_weight_f32(void *stream, const float *weight, int cin, float *wpack);
int upsnet_stem_pool_f32(void *stream, const float *x4, int batch, int height, int width, const float *wpack, const float *bias, float *out);
/* The backbone stem in one launch on the bf16 matrix cores (upsnet/models/resnet.py:347-356 in the bf16 mode): convolution 7x7 /
 * stride 2 / pad 3 (Cin <= 4 -> 64, frozen BN folded: + bias) + ReLU + max-pool 3x3 / stride 2 / pad 1. x4 [N,H,W,4] fp32 (RGB + a zero
 * channel: upsnet_image_to_nhwc4 / upsnet_prep_image_u8), wpack = upsnet_stem_pool_pack_weight_bf16(weight [64,Cin,7,7]) (28 KiB),
 * bias [64] or NULL, out [N,Hp,Wp,64] bf16, Hc = (H - 1) / 2 + 1, Hp = (Hc - 1) / 2 + 1 (likewise the width). The convolution result
 * is rounded to bf16 before the pool; the image is rounded to bf16 on the way into LDS. */
int upsnet_stem_pool_pack_weight_bf16(void *stream, const float *weight, int cin, void *wpack);
int upsnet_stem_pool_bf16(void *stream, const float *x4, int batch, int height, int width, const void *wpack, const float *bias, void *out);
/* ConvTranspose2d(kernel 2, stride 2, pad 0) (+ bias, + ReLU) of a bf16 NHWC map on the bf16 matrix cores (the mask head's
 * upsampling layer, upsnet/models/rcnn.py:132-133, in the bf16 mode): one GEMM [N H W, Cin] x [Cin, 4 Cout] with a scatter epilogue.
 * x [N,H,W,Cin] bf16; wpack_hi = upsnet_conv_pack_weight_bf16 of the [4 Cout, Cin, 1, 1] matrix whose rows are ordered (ky, kx, c),
 * ldw = 4 Cout; bias [Cout] or NULL; out [N,2H,2W,Cout] fp32 (out_bf16 = 0) or bf16. Cin % 64 == 0, Cout % 32 == 0. */
int upsnet_deconv2x2_nhwc_bf16(void *stream, const void *x, int batch, int height, int width, int Cin, const void *wpack_hi, int ldw,
                               const float *bias, int Cout, int relu, void *out, int out_bf16);

/* One identity bottleneck of the backbone (upsnet/models/resnet.py:84-100: conv1 1x1 C -> Cm, conv2 3x3 Cm -> Cm, conv3 1x1 Cm -> C,
 * C = 4 Cm, stride 1, no projection; frozen BN folded; out = relu(conv3(relu(conv2(relu(conv1(x))))) + x)) as ONE launch on the bf16
 * matrix cores -- the bf16 mode of BASELINE.json configs[2]; the intermediates never leave the LDS. x, out: [N,H,W,C] bf16 NHWC;
 * cmid in {64, 128, 256, 512}; w1 / w2 / w3: bf16 in MFMA-fragment order [out channel / 32][k / 16][64 lanes][8]
 * (element (cb, ks, lane, e) = W[cb 32 + lane % 32][ks 16 + (lane / 32) 8 + e], k = input channel for the 1x1 layers and
 * (ky 3 + kx) Cm + c for the 3x3 layer); b1, b2 [Cm], b3 [C] fp32. Every intermediate is rounded to bf16 where the three separate
 * launches of upsnet_conv2d_nhwc_bf16 round it. */
int upsnet_bottleneck_bf16(void *stream, const void *x, void *out, int batch, int height, int width, int cmid, const void *w1,
                           const void *w2, const void *w3, const float *b1, const float *b2, const float *b3);

/* 7x7/2 stem (upsnet/models/resnet.py:347-356, conv1 + frozen BN + ReLU): Cin <= 4 input given as NHWC with 4 channels
 * (x [N,H,W,4], 4th channel ignored by zero weights; see upsnet_image_to_nhwc4 / upsnet_prep_image_u8). One K slab of the
 * implicit GEMM is one kernel row: 8 consecutive pixels x 4 channels. wpack [KH*32, ldw] from upsnet_conv_pack_weight_stem
 * (weight [Cout,Cin,KH,KW], KW <= 8); out [N,Ho,Wo,Cout] NHWC; bias/ReLU fused. */
int upsnet_conv2d_stem_nhwc4_f32(void *stream, const float *x, int batch, int height, int width, const float *wpack,
                                 int ldw, const float *bias, int Cout, int KH, int KW, int stride, int pad, int relu,
                                 float *out);
int upsnet_conv_pack_weight_stem(void *stream, const float *weight, int cout, int cin, int kh, int kw, int ldw, float *wpack);

/* nn.ConvTranspose2d(Cin, Cout, 2, 2, 0) (+ bias + ReLU) of the mask head (upsnet/models/rcnn.py:60,84) as ONE GEMM with
 * 4*Cout columns (dy, dx, co) whose epilogue stores column (dy,dx,co) of input pixel (h,w) at output pixel (2h+dy, 2w+dx):
 * x [N,H,W,Cin] NHWC -> out [N,2H,2W,Cout] NHWC. wpack [Cin, ldw >= 4*Cout] from upsnet_deconv2x2_pack_weight
 * (weight [Cin,Cout,2,2], the PyTorch layout). */
int upsnet_deconv2x2_nhwc_f32(void *stream, const float *x, int batch, int height, int width, int Cin, const float *wpack,
                              int ldw, const float *bias, int Cout, int relu, float *out);
int upsnet_deconv2x2_pack_weight(void *stream, const float *weight, int cin, int cout, int ldw, float *wpack);

/* The same transposed convolution on the lean 1x1 GEMM kernel (csrc/conv1x1.hip, scatter epilogue): x [N,H,W,Cin] NHWC ->
 * out [N,2H,2W,Cout] NHWC. wpack: upsnet_dcn_pack_weight(W', 4*Cout, Cin, 1, 1) of the [4*Cout, Cin, 1, 1] matrix W' whose rows are
 * (dy, dx, co) = weight[ci, co, dy, dx]; bias4 = the bias repeated for the four (dy, dx), [4*Cout], or NULL. Cin % 32 == 0,
 * Cout % 32 == 0. Same fp32 MFMA arithmetic and K order as upsnet_conv1x1_frag_nhwc_f32. Replaces the reference's
 * nn.ConvTranspose2d(dim, dim, 2, 2, 0) + ReLU of the mask head (upsnet/models/rcnn.py:132-133). */
int upsnet_deconv2x2_frag_nhwc_f32(void *stream, const float *x, float *out, int batch, int height, int width, int Cin,
                                   const float *wpack, const float *bias4, int Cout, int relu);

/* Development knob for A/B measurements: force_tile = 0 auto, 1: 128x128, 2: 128x64, 3: 128x32, 4: 64x128, 5: 64x64,
 * 6: 64x64 with 64-channel K slabs (pixels x output channels per workgroup). winograd_tiles = 0 auto, 32 / 64: 2x2 tiles per
 * workgroup of the Winograd kernel. Not needed in production. */
void upsnet_conv_tuning(int winograd_tiles, int force_tile);

/* weight [Cout, Cin, kh, kw] (nn.Conv2d layout) -> wpack [kh*kw*Cin, ldw] (tap-major rows, zero-padded columns). */
int upsnet_conv_pack_weight(void *stream, const float *weight, int cout, int cin, int kh, int kw, int ldw, float *wpack);

/* 1x1 convolution (stride 1 / 2) as a lean fp32 MFMA GEMM (csrc/conv1x1.hip): the 1x1 layers of the ResNet bottlenecks
 * (upsnet/models/resnet.py:53-100: conv1 / conv3 / downsample) and the FPN laterals with their top-down add (fpn.py:78-104).
 * out = relu?(conv1x1(x; stride) + bias + residual); x [N,H,W,Cin] NHWC, out [N,Ho,Wo,Cout] NHWC (Ho = (H-1)/stride + 1);
 * residual like out, or -- residual_up != 0 -- [N,Ho/2,Wo/2,Cout] read through a nearest x2 upsampling. Cin % 32 == 0.
 * wpack: upsnet_dcn_pack_weight(weight [Cout,Cin,1,1], cout, cin, 1, 1) (MFMA fragment order, read straight from L2).
 * Weights must be FINITE: when Cin / 32 (or a split-K slice) is odd the K walk runs one padding step that multiplies zero activations
 * by the last weight slab (0 x Inf would be NaN; an exact zero otherwise).
 * upsnet_conv1x1_tuning: development knob (0 auto, 64 / 128: output channels per workgroup). */
int upsnet_conv1x1_frag_nhwc_f32(void *stream, const float *x, const float *residual, float *out, int batch, int height, int width,
                                 int Cin, const float *wpack, const float *bias, int Cout, int stride, int relu, int residual_up);
void upsnet_conv1x1_tuning(int bn);
/* Two 1x1 convolutions of the same input in one launch -- conv1 and the projection shortcut (`downsample`) of a stage's first bottleneck
 * (upsnet/models/resnet.py:53-100 reads x twice): out_a [N,Ho,Wo,cout_a] from rows [0, cout_a) of the concatenated weight, out_b
 * [N,Ho,Wo,cout_b] from the rest; wpack = upsnet_dcn_pack_weight of the concatenated [cout_a + cout_b, Cin, 1, 1] weight, bias = both
 * biases concatenated (or NULL), cout_a % 32 == 0. Bit-identical to two upsnet_conv1x1_frag_nhwc_f32 launches. */
int upsnet_conv1x1_siblings_nhwc_f32(void *stream, const float *x, float *out_a, float *out_b, int batch, int height, int width, int Cin,
                                     const float *wpack, const float *bias, int cout_a, int cout_b, int stride, int relu_a, int relu_b);
/* development knob: waves per workgroup of the 32-pixel form of upsnet_conv1x1_pair_nhwc_f32 (8: two per SIMD, default; 4). */
void upsnet_conv1x1_pair32_tuning(int waves);

/* Residency table (csrc/residency.h): at most `cap` workgroups of a kernel per CU, so that a kernel of another stream -- the other image
 * in flight -- can live on the CU beside it. kernel: 0 conv1x1_frag (every mode), 1 conv1x1_pair, 2 conv1x1_pair32, 3 conv1x1_ksw,
 * 4 conv_wino16<.,32,64>, 5 conv_wino16<.,32,32>, 6 dcn_fused_f32; -1: all of them. cap: 0 the plain launch (the state after loading),
 * 1..8, or -1: the measured default of that kernel. The launcher enforces a cap by asking for more dynamic LDS than the kernel uses
 * (160 KiB per CU, 1280-byte granules); kernel code and results do not change by a bit. A cap at or above what the kernel's own
 * registers / LDS admit adds nothing. The model sets (-1, -1) while it captures the graphs of two or more images in flight and (-1, 0)
 * afterwards; eager launches are never capped.
 * upsnet_residency_pad_bytes: the dynamic LDS added for `cap` to a workgroup of static_lds + dynamic_lds bytes (the launchers' arithmetic).
 * upsnet_residency_last_dynamic_lds: dynamic LDS of the most recent launch of a covered kernel (tests). */
int upsnet_residency_tuning(int kernel, int cap);
size_t upsnet_residency_pad_bytes(int cap, size_t static_lds, size_t dynamic_lds);
int upsnet_residency_last_dynamic_lds(void);

/* 3x3 / stride 1 / pad 1 convolution (+ bias, ReLU) of up to 5 NHWC maps sharing weights by Winograd F(4x4, 3x3) (csrc/conv_wino36.hip,
 * r11 / r12): 36 multiplies per 16 outputs, 0.5625 of the F(2x2) kernel's matrix work. Interpolation points {0, 3/4, -3/4, 3/2, -3/2, inf}:
 * within rtol = atol = 1e-4 of float64 on the model's layers, measured worst error 0.07-0.15 of that bound at the model's shapes (3-4x the
 * F(2x2) kernel's 0.014-0.032; tools/bench_winograd36.py), asserted <= 0.35 in tests/test_conv_gpu.py (small maps and the real 1024x2048
 * sizes). H, W of any size (maps with H < 4 take the bounds-flagged loads throughout). The
 * contract of upsnet_conv2d_winograd_nhwc_f32 without a residual; Cin % 32 == 0; wpack (36 * Cin * ldw floats, ldw = Cout rounded up to
 * 64) from upsnet_conv_pack_weight_winograd36 (weight [Cout, Cin, 3, 3]). */
int upsnet_conv2d_winograd36_nhwc_f32(void *stream, int nseg, const float *const x[], float *const out[], const int batch[],
                                      const int height[], const int width[], int Cin, const float *wpack, int ldw, const float *bias,
                                      int Cout, int relu);
int upsnet_conv_pack_weight_winograd36(void *stream, const float *weight, int cout, int cin, int ldw, float *wpack);
/* r13: upsnet_conv2d_winograd36_nhwc_f32 of ONE map with the channel walk of every tile split over `ksplit` (2..8, <= Cin / 16) workgroups: each
 * stores the output transform of its partial sums, the shared reduce / epilogue kernel adds them in a fixed order (+ bias, ReLU;
 * bit-repeatable). For maps with fewer 32-tile x 64-channel workgroups than CUs (res3 / res4 conv2, FPN P4 at 1024x2048). workspace:
 * upsnet_conv2d_winograd36_splitk_workspace_bytes(batch, height, width, Cout, ksplit) bytes, caller-allocated. */
size_t upsnet_conv2d_winograd36_splitk_workspace_bytes(int batch, int height, int width, int Cout, int ksplit);
int upsnet_conv2d_winograd36_nhwc_f32_splitk(void *stream, const float *x, float *out, int batch, int height, int width, int Cin,
                                             const float *wpack, int ldw, const float *bias, int Cout, int relu, int ksplit, void *workspace);

/* 1x1 convolution (stride 1 / 2; + bias, + residual, ReLU) on SMALL tiles (csrc/conv1x1_ksw.hip, r13): `v_mfma_f32_16x16x4_f32` fragments,
 * every wave of a workgroup holds the whole tile_pixels x tile_channels tile and walks a quarter of K straight from the NHWC map (no LDS /
 * barrier in the K loop); the four partial tiles are added in LDS in a fixed order ((w0 + w1) + (w2 + w3): bit-repeatable, independent
 * of the batch size for a given tile). For maps the 64-pixel tiles of upsnet_conv1x1_frag_nhwc_f32 do not spread evenly over the CUs
 * (UPSNet-101-DCN at 800x1333: 4200-pixel maps; the layers replaced are the bottlenecks' conv1 / conv3, upsnet/models/resnet.py:53-153).
 * Tiles (pixels x channels of a workgroup; anything else is an error): split_n == 0 -- 16 x 64, 32 x 32, 32 x 64, 64 x 64, the waves split K
 * as described; split_n == 1 -- 16 x 256, 32 x 128, 32 x 256: the four waves split the tile's CHANNELS instead and each walks all of K (no
 * reduction; for a short K walk into many channels, a bottleneck's conv3). x [N,H,W,Cin] NHWC, out [N,Ho,Wo,Cout] NHWC,
 * residual like out or NULL; Cin % 16 == 0, Cout % 4 == 0, all pointers 16-byte aligned. wpack: upsnet_conv1x1_ksw_packed_weight_floats
 * floats from upsnet_conv1x1_ksw_pack_weight (weight [Cout, Cin]). Finite weights assumed (a K step beyond a wave's share multiplies
 * zeros by the last valid weights). upsnet_conv1x1_ksw_tuning(1000 split_n + 100 RB + CB of a wave's tile): development knob forcing an instance (0: the caller's). */
size_t upsnet_conv1x1_ksw_packed_weight_floats(int cout, int cin);
int upsnet_conv1x1_ksw_pack_weight(void *stream, const float *weight, int cout, int cin, float *wpack);
int upsnet_conv1x1_ksw_nhwc_f32(void *stream, const float *x, const float *residual, float *out, int batch, int height, int width, int Cin,
                                const float *wpack, const float *bias, int Cout, int stride, int relu, int tile_pixels, int tile_channels,
                                int split_n);
void upsnet_conv1x1_ksw_tuning(int tile);

/* 3x3 / stride 1 / pad 1 convolution (+ bias, ReLU) into Cout <= 32 channels on the small-tile scheme of upsnet_conv1x1_ksw_nhwc_f32
 * (csrc/conv1x1_ksw.hip, r13): 16-pixel x 32-channel workgroups, the (tap, channel) walk split over the four waves, no LDS in the K loop.
 * Replaces the separate launch pair (split-K general kernel + reduce) of the 18-channel offset predictors of the deformable bottlenecks on
 * small maps (conv2_offset, upsnet/models/resnet.py:102-153). x [N,H,W,Cin] NHWC, out [N,H,W,Cout] NHWC, Cin % 16 == 0; wpack:
 * upsnet_conv3x3_ksw_packed_weight_floats(Cin) floats from upsnet_conv3x3_ksw_pack_weight (weight [Cout, Cin, 3, 3]). Finite weights
 * assumed. Fixed summation order for a given pixel count (bit-repeatable; the number of waves that share a tile's walk -- 4, 8 or 16 --
 * follows the tile count, so a pixel's bits may differ between launches of different sizes: not for ROI batches). */
size_t upsnet_conv3x3_ksw_packed_weight_floats(int cin);
int upsnet_conv3x3_ksw_pack_weight(void *stream, const float *weight, int cout, int cin, float *wpack);
int upsnet_conv3x3_ksw_nhwc_f32(void *stream, const float *x, float *out, int batch, int height, int width, int Cin, const float *wpack,
                                const float *bias, int Cout, int relu);

/* upsnet_conv1x1_frag_nhwc_f32 with the K walk of every tile split over `ksplit` (2..16) workgroups + the shared reduce / epilogue
 * kernel (bias, residual, ReLU; fixed summation order: bit-repeatable). For maps whose tile count does not spread evenly over the CUs:
 * a workgroup of this kernel keeps all four SIMDs of its CU at the MFMA rate, so a launch lasts (most workgroups on one CU) x (one K
 * walk) -- 264 tiles on 256 CUs take two walks, 264 x 4 quarter walks take five quarters (models/hipconv.py: UPSNET_CONV1X1_BALANCE).
 * workspace: upsnet_conv1x1_splitk_workspace_bytes(batch, Ho, Wo, Cout, ksplit) bytes, caller-allocated. No residual_up. */
size_t upsnet_conv1x1_splitk_workspace_bytes(int batch, int out_height, int out_width, int Cout, int ksplit);
int upsnet_conv1x1_frag_nhwc_f32_splitk(void *stream, const float *x, const float *residual, float *out, int batch, int height, int width,
                                        int Cin, const float *wpack, const float *bias, int Cout, int stride, int relu, int ksplit,
                                        void *workspace);

/* Two chained 1x1 convolutions of consecutive bottlenecks in ONE launch (csrc/conv1x1_pair.hip) -- the tail of block b and the
 * head of block b+1 of Bottleneck.forward (upsnet/models/resnet.py:53-100):
 *     out1 = relu(conv1x1(x; w3) + bias3 + residual)      x [pixels, C0], residual / out1 [pixels, C1]   (NHWC, pixels = N*H*W)
 *     out2 = relu(conv1x1(out1; w1) + bias1)              out2 [pixels, C2]
 * Both results are bit-identical to two upsnet_conv1x1_frag_nhwc_f32 launches; out1 is not read back from HBM.
 * w3pack / w1pack: upsnet_dcn_pack_weight(weight, cout, cin, 1, 1). Supported: (C0, C2) = (64, 64), (128, 128) or (256, 256), C1 % 128 == 0 (the res2, res3 and -- on 32-pixel tiles -- res4 stages). */
int upsnet_conv1x1_pair_nhwc_f32(void *stream, const float *x, const float *residual, float *out1, float *out2, long pixels, int C0,
                                 const float *w3pack, const float *bias3, int C1, const float *w1pack, const float *bias1, int C2);

/* ============================== NMS ============================== */

/* Drop-in for `_nms` (upsnet/nms/gpu_nms.hpp:15, nms_kernel.cu:97-150): HOST pointers in and out,
 * boxes already sorted by descending score, keep_out = indices into the sorted array. */
int upsnet_nms_host(int *keep_out_host, int *num_out_host, const float *boxes_host, int boxes_num,
                    int boxes_dim, float nms_overlap_thresh, int device_id);

/* Batched device-resident hard NMS: P independent problems in one set of launches, no host round trip.
 * Replaces gpu_nms (upsnet/nms/gpu_nms.pyx:23-38) including its score sort: visiting order is
 * (score desc, index desc), the pinned meaning of scores.argsort()[::-1].
 *   boxes [P,nmax,4], scores [P,nmax], counts [P] (device int32, counts[p] <= nmax <= 8192)
 *   pre_removed (optional) [P,nmax] uint8: boxes dropped before NMS (min-size filter)
 *   keep_idx [P,nmax] int32 out (original indices, visiting order; rows >= keep_cnt[p] unspecified), keep_cnt [P] int32 out
 *   workspace: upsnet_nms_workspace_bytes(P, nmax) bytes. */
size_t upsnet_nms_workspace_bytes(int num_problems, int nmax);
int upsnet_nms_batched(void *stream, const float *boxes, const float *scores, const int *counts,
                       const uint8_t *pre_removed, int num_problems, int nmax, float thresh, int *keep_idx,
                       int *keep_cnt, void *workspace);

/* Development knob of the greedy scan: 0 = default (row-layout scan for problems of <= 1024 boxes, general scan reading L2 above
 * that), 1 = general scan on an LDS copy of the mask (<= 1024 boxes), 2 = general scan reading L2 at every size. Same keep lists. */
void upsnet_nms_tuning(int lds_staging);

/* cpu_nms (upsnet/nms/cpu_nms.pyx:29-80, behind cpu_nms_wrapper, upsnet/nms/nms.py:37-40) on the device: same layout, visiting
 * order and IoU expression as upsnet_nms_batched, but suppression at `overlap >= thresh` (:77) with `thresh` a double (a Python
 * float in the reference's compiled module; the fp32 overlap is compared in double). */
int upsnet_cpu_nms_batched(void *stream, const float *boxes, const float *scores, const int *counts, int num_problems,
                           int nmax, double thresh, int *keep_idx, int *keep_cnt, void *workspace);

/* Batched device soft-NMS = cpu_soft_nms (upsnet/nms/cpu_nms.pyx:91-196), P independent problems (RPN levels / classes) per
 * launch, one workgroup each, state resident in LDS for nmax <= 4096. Bit-compatible with the compiled reference on the
 * returned prefix (pinned: tests/test_ref_cpu_nms.py):
 *   boxes [P,nmax,5] in/out (x1,y1,x2,y2,score; rows >= n_out[p] unspecified), inds [P,nmax] int64 out (original index of each
 *   surviving row; rows >= n_out[p] unspecified), counts [P] device int32 (valid rows per problem; NULL = nmax everywhere), n_out [P] device int32.
 *   method: 0 hard, 1 linear, 2 gaussian. workspace: upsnet_soft_nms_batched_workspace_bytes(P, nmax) (may be NULL when
 *   nmax <= 4096). */
size_t upsnet_soft_nms_batched_workspace_bytes(int num_problems, int nmax);
int upsnet_soft_nms_batched(void *stream, float *boxes, int64_t *inds, const int *counts, int num_problems, int nmax,
                            float sigma, float Nt, float threshold, int method, int *n_out, void *workspace);

/* Single problem: upsnet_soft_nms_batched with P = 1 and all n rows valid. */
size_t upsnet_soft_nms_workspace_bytes(int n);
int upsnet_soft_nms(void *stream, float *boxes, int64_t *inds, int n, float sigma, float Nt, float threshold,
                    int method, int *n_out, void *workspace);

/* ============================== RPN proposals ============================== */

/* Replaces PyramidProposalFunction.forward + PyramidProposal.forward
 * (upsnet/operators/functions/pyramid_proposal.py:62-222, modules/pyramid_proposal.py:61-67) with
 * individual_proposals=True (every shipped yaml; the joint branch is upsnet_pyramid_proposals_joint_strided below), entirely on device.
 *   cls_prob[l] [A,H_l,W_l] NCHW (A anchors), bbox_pred[l] [4A,H_l,W_l] NCHW  (HOST arrays of pointers)
 *   anchors_host [nlev*A*4] base anchors (generate_anchors), strides_host [nlev]
 *   im_info (device) [3] = (H, W, scale)
 *   rois_out [post_nms_top_n,5], scores_out [post_nms_top_n], num_out device int32
 *   workspace: upsnet_proposal_workspace_bytes(...) bytes. */
size_t upsnet_proposal_workspace_bytes(int nlev, const int *heights_host, const int *widths_host, int num_anchors,
                                       int pre_nms_top_n, int post_nms_top_n);
int upsnet_pyramid_proposals(void *stream, int nlev, const float *const cls_prob[], const float *const bbox_pred[],
                             const int *heights_host, const int *widths_host, const int *strides_host,
                             const float *anchors_host, int num_anchors, const float *im_info, int pre_nms_top_n,
                             int post_nms_top_n, float nms_thresh, float min_size, float *rois_out,
                             float *scores_out, int *num_out, void *workspace);

/* Same operator on strided inputs, so that channel slices of NHWC maps (the RPN head's [H,W,15] output: 3 scores + 12 deltas per
 * pixel) are consumed in place instead of being copied to NCHW first: element (channel c, pixel) of level l's score map is
 * cls_prob[l][c * cls_chan_stride[l] + pixel * cls_pix_stride[l]], likewise for the deltas. A NULL stride array means NCHW
 * (channel stride H*W, pixel stride 1). */
int upsnet_pyramid_proposals_strided(void *stream, int nlev, const float *const cls_prob[], const float *const bbox_pred[],
                                     const long *cls_chan_stride, const long *cls_pix_stride, const long *box_chan_stride,
                                     const long *box_pix_stride, const int *heights_host, const int *widths_host,
                                     const int *strides_host, const float *anchors_host, int num_anchors, const float *im_info,
                                     int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float min_size, float *rois_out,
                                     float *scores_out, int *num_out, void *workspace);
/* r13: the same + roi_order_out (int[post_nms_top_n] or NULL): the workgroup -> ROI table of upsnet_fpn_roi_align_forward_ordered for these
 * rois (see upsnet_fpn_roi_order), written by the launch that ranks them -- no launch of its own. post_nms_top_n <= 2048 when given. */
int upsnet_pyramid_proposals_strided_ordered(void *stream, int nlev, const float *const cls_prob[], const float *const bbox_pred[],
                                     const long *cls_chan_stride, const long *cls_pix_stride, const long *box_chan_stride,
                                     const long *box_pix_stride, const int *heights_host, const int *widths_host,
                                     const int *strides_host, const float *anchors_host, int num_anchors, const float *im_info,
                                     int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float min_size, float *rois_out,
                                     float *scores_out, int *num_out, void *workspace, int *roi_order_out);

/* individual_proposals=False -- the DEFAULT of the reference's constructors (functions/pyramid_proposal.py:26,
 * modules/pyramid_proposal.py:24) -- i.e. the joint branch functions/pyramid_proposal.py:181-208: every anchor of every level is decoded,
 * clipped and size-filtered (:132-141), the survivors are concatenated (:176-177) and ranked jointly (`scores.argsort()[::-1]`: equal
 * scores -> higher concatenation index first), the first pre_nms_top_n go through ONE NMS, the first post_nms_top_n kept boxes are
 * the result. Same arguments and workspace as upsnet_pyramid_proposals_strided; pre_nms_top_n <= 8192.
 *   rois_out [post_nms_top_n,5] / scores_out: the kept boxes in NMS visiting order, zero rows behind; num_out = their number.
 * NOT done here: the reference then pads the list back to post_nms_top_n rows with `np.random.choice(keep, ...)` (:205-207, numpy's
 * global generator -- host state); upsnet_amd/operators/functions/pyramid_proposal.py draws those indices on the host from the
 * same generator (identical stream) and gathers the rows. */
int upsnet_pyramid_proposals_joint_strided(void *stream, int nlev, const float *const cls_prob[], const float *const bbox_pred[],
                                           const long *cls_chan_stride, const long *cls_pix_stride, const long *box_chan_stride,
                                           const long *box_pix_stride, const int *heights_host, const int *widths_host,
                                           const int *strides_host, const float *anchors_host, int num_anchors, const float *im_info,
                                           int pre_nms_top_n, int post_nms_top_n, float nms_thresh, float min_size, float *rois_out,
                                           float *scores_out, int *num_out, void *workspace);

/* ============================== Detection selection (MaskROI) ============================== */

/* Replaces MaskROI.forward (upsnet/operators/modules/mask_roi.py:36-146): decode + clip, per-class (or
 * class-agnostic) score threshold, NMS, global top-max_det; dummy ROI when nothing survives.
 *   rois [N,5], bbox_delta [N,4*C], cls_prob [N,C], num_rois_dev optional device count
 *   boxes_out [cap,5], scores_out [cap], cls_out [cap] int64, src_out [cap] int32 (ROI row of each det),
 *   num_out device int32; cap = upsnet_mask_roi_capacity(N, C, class_agnostic). Rows >= *num_out of the four outputs are
 *   unspecified (consumers read the first *num_out). */
int upsnet_mask_roi_capacity(int num_rois, int num_classes, int class_agnostic);
size_t upsnet_mask_roi_workspace_bytes(int num_rois, int num_classes, int class_agnostic);
int upsnet_mask_roi(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                    const int *num_rois_dev, int num_classes, const float *im_info, int class_agnostic,
                    float score_thresh, float nms_thresh, int max_det, const float reg_weights_host[4],
                    float *boxes_out, float *scores_out, int64_t *cls_out, int *src_out, int *num_out,
                    void *workspace);
/* The same with MaskROI's `clip_boxes` constructor argument (mask_roi.py:25,53-54): clip_boxes = 0 skips clip_boxes(), the
 * decoded boxes reach the NMS and the output unclipped; upsnet_mask_roi is clip_boxes = 1. */
int upsnet_mask_roi_ex(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                       const int *num_rois_dev, int num_classes, const float *im_info, int class_agnostic, int clip_boxes,
                       float score_thresh, float nms_thresh, int max_det, const float reg_weights_host[4],
                       float *boxes_out, float *scores_out, int64_t *cls_out, int *src_out, int *num_out,
                       void *workspace);

/* The reference runs the mask head on the per-class detections AND on the class-agnostic "panoptic" detections
 * (upsnet/models/resnet_upsnet.py:190,215). Both are selections from the same (ROI row, class) table, and every ROI goes
 * through the mask head independently, so a panoptic detection that is also a per-class detection gets bit-identical
 * logits. Given the src/cls outputs of two upsnet_mask_roi calls (set A, set B) this entry writes, for every b in B,
 * map_out[b] = its row in the concatenation [A ; unmatched of B], compacts the unmatched boxes of B (in order) into
 * extra_boxes [cap_b,5] and their count into num_extra (device int). One mask-head pass over [A ; extra] then serves both.
 * map_out rows >= *num_b and extra_boxes rows >= *num_extra are unspecified. */
int upsnet_mask_roi_dedup(void *stream, const int *a_src, const int64_t *a_cls, const int *num_a, int cap_a, const int *b_src,
                          const int64_t *b_cls, const float *b_boxes, const int *num_b, int cap_b, int *map_out,
                          float *extra_boxes, int *num_extra);

/* out[k, :] = mask_logit[row[k], cls[k], :] for k < K: the class plane of each panoptic detection's mask logits
 * (upsnet/models/resnet_upsnet.py:215-221) as one gather. mask_logit is addressed by element strides (stride_n per ROI, stride_c
 * per class, stride_e per spatial element: NHWC or NCHW); row int32 [K], cls int64 [K] are clamped to the valid range; out [K, hw]. */
int upsnet_mask_logit_gather(void *stream, const float *mask_logit, int n_rows, int num_classes, int hw, long stride_n,
                             long stride_c, long stride_e, const int *row, const int64_t *cls, int K, float *out);

/* ============================== Panoptic head ============================== */

/* Replaces MaskRemoval.forward's selection (upsnet/operators/modules/mask_removal.py:50-93):
 *   mask_rois [m,4], cls_prob [m], mask_logit [m,ms,ms], cls_idx [m] int64 (1-based; 0 = dummy)
 *   keep_inds [m] int64 out (visiting order), num_keep device int32 (>=1: the reference's [0] fallback)
 *   real_keep device int32: 0 when the fallback fired (then the single mask plane is all zeros).
 *   m_dev (optional device int32): the arrays have capacity m and *m_dev (<= m) valid rows -- lets the call sit inside a
 *   HIP graph before the host knows the detection count; NULL: all m rows are valid. */
size_t upsnet_mask_removal_workspace_bytes(int m, int num_thing_classes, int height, int width);
int upsnet_mask_removal(void *stream, const float *mask_rois, const float *cls_prob, const float *mask_logit,
                        const int64_t *cls_idx, int m, const int *m_dev, int mask_size, int num_thing_classes, int height, int width,
                        double fraction_threshold, int64_t *keep_inds, int *num_keep, int *real_keep,
                        void *workspace);

/* Tail of the fixed-capacity forward (models/resnet_upsnet.py): kept_cls[i] = cls[keep[i]], kept_scores[i] = scores[keep[i]] for the
 * kept panoptic detections (panoptic_cls_inds / panoptic_cls_probs of upsnet/models/resnet_upsnet.py:242-247; rows past *num_keep read
 * row 0) and counters = {*det_num, *pan_num, *extra_num, *num_keep}: one launch instead of clamp + 2 index_select + 2 cat. */
int upsnet_panoptic_tail_pack(void *stream, const int64_t *keep, const int *num_keep, int K, const int64_t *cls, const float *scores,
                              const int *det_num, const int *pan_num, const int *extra_num, int64_t *kept_cls, float *kept_scores,
                              int *counters);

/* Materialise MaskRemoval's mask_energy [k,H,W] (mask_removal.py:86) for the kept instances. */
int upsnet_mask_paste(void *stream, const float *mask_rois, const float *mask_logit, const int64_t *keep_inds,
                      const int *num_keep, const int *real_keep, int kmax, int mask_size, int height, int width,
                      float *mask_energy);

/* Materialise SegTerm's seg_inst_energy [k,H,W] (upsnet/operators/modules/unary_logits.py:95-103).
 * boxes [k,4] image coords (already scaled), cls [k] int64, class_map [num_classes] int64. */
int upsnet_seg_term(void *stream, const float *fcn_output, int num_seg, int height, int width, const float *boxes,
                    const int64_t *cls, const int64_t *class_map, int k, float *seg_inst);

/* Fused parameter-free panoptic head (upsnet/models/resnet_upsnet.py:223-243 + SegTerm + mask paste):
 * one pass over fcn_output, nothing materialised.
 *   fcn_output [S,H,W] planar; mask_rois [m,5] (col 0 = batch), mask_logit [m,ms,ms], cls_idx [m] int64,
 *   keep_inds/num_keep/real_keep from upsnet_mask_removal; class_map [num_classes] int64
 *   pan_out [H,W] int64, sem_out [H,W] int64 or NULL (argmax over S, resnet_upsnet.py:213). */
int upsnet_panoptic_fuse(void *stream, const float *fcn_output, int num_seg, int height, int width, int num_stuff,
                         const float *mask_rois, const float *mask_logit, const int64_t *cls_idx,
                         const int64_t *keep_inds, const int *num_keep, const int *real_keep, int kmax,
                         int mask_size, const int64_t *class_map, int enable_void, int64_t *pan_out,
                         int64_t *sem_out);

/* Tail of the semantic head (upsnet/models/fcn.py:94-100: upsample x2/x4/x8, concat, 1x1 `score` conv), with the linear
 * 1x1 convolution commuted below the bilinear upsampling: part[l] = W[:, 128 l:128 (l+1)] . y_l at level l's own
 * resolution, NHWC [height >> l, width >> l, num_seg] (made with upsnet_conv2d_nhwc_f32); this entry computes
 *   score[y,x,s] = bias[s] + part[0][y,x,s] + sum_{l>=1} bilinear_up_{2^l}(part[l])[y,x,s]   (align_corners = False)
 * into score [height, width, num_seg] NHWC. bias may be NULL. 1 <= nlev <= 4. */
int upsnet_fcn_score_combine(void *stream, int nlev, const float *const part[], int num_seg, int height, int width,
                             const float *bias, float *score);

/* Same as upsnet_panoptic_fuse (enable_void branch) but ALSO fuses FCNHead's x4 bilinear upsampling
 * (F.interpolate(score, None, 4, 'bilinear', align_corners=False), upsnet/models/fcn.py:101): takes the low-resolution
 * fcn_score [S,Hs,Ws] (score_nhwc = 0) or [Hs,Ws,S] (score_nhwc = 1); label maps are [Hs*scale, Ws*scale]. */
int upsnet_panoptic_fuse_up(void *stream, const float *fcn_score, int score_nhwc, int num_seg, int score_h, int score_w,
                            int scale, int num_stuff, const float *mask_rois, const float *mask_logit,
                            const int64_t *cls_idx, const int64_t *keep_inds, const int *num_keep, const int *real_keep,
                            int kmax, int mask_size, const int64_t *class_map, int64_t *pan_out, int64_t *sem_out);

/* upsnet_panoptic_fuse_up with the confidence of every pixel (the reference keeps the arg-max only). The rule:
 *   - z, the panoptic logits of a pixel of the [Hs*scale, Ws*scale] map, are exactly those upsnet_panoptic_fuse_up compares: the
 *     num_stuff stuff logits (the x4 bilinear upsampling of the score, fp32 without FMA); for each of the k = *num_keep kept instances in
 *     index order seg_inst + mask_energy, which is exactly 0 where the instance touches neither its box nor its mask (with
 *     *real_keep == 0 the one dummy channel has no mask energy, as in the reference); the void logit max(thing channels) - max_j seg_inst_j;
 *   - P = softmax(z) (the reference's training loss is over exactly these channels, resnet_upsnet.py:234-243);
 *   - conf = P[winner], the winner being the label pan_out gets (255: the void channel). The winner is a maximum of z, so
 *     conf = 1 / sum_c exp(z_c - z_max), in fp32, every one of the k instance channels included;
 *   - conf_out = (unsigned)(conf * 255.0f + 0.5f), one byte per pixel.
 * conf_out uint8 [Hs*scale, Ws*scale], 4-byte aligned. pan_out and sem_out are bit-equal to upsnet_panoptic_fuse_up's; one launch of
 * a kernel of its own, so the label-only kernel is what it was. Everything else as upsnet_panoptic_fuse_up. */
int upsnet_panoptic_fuse_up_conf(void *stream, const float *fcn_score, int score_nhwc, int num_seg, int score_h, int score_w,
                                 int scale, int num_stuff, const float *mask_rois, const float *mask_logit,
                                 const int64_t *cls_idx, const int64_t *keep_inds, const int *num_keep, const int *real_keep,
                                 int kmax, int mask_size, const int64_t *class_map, int64_t *pan_out, int64_t *sem_out,
                                 unsigned char *conf_out);

/* Reference-shaped fusion on materialised planes (resnet_upsnet.py:234-243):
 * seg_inst, mask_energy [k,H,W]. */
int upsnet_panoptic_argmax(void *stream, const float *fcn_output, int num_seg, int height, int width, int num_stuff,
                           const float *seg_inst, const float *mask_energy, int k, int enable_void,
                           int64_t *pan_out);

/* ============================== Unified panoptic result (the step after the path) ============================== */

/* BaseDataset.get_unified_pan_result (upsnet/dataset/base_dataset.py:332-371) for one image, on the device:
 *   pan [H,W] int64 panoptic label map of the network (stuff ids 0..id_last_stuff, instance j -> id_last_stuff+1+j, 255 void),
 *   seg [H,W] int64 semantic argmax map, cls_inds [num_inst] int64 (1-based thing class of instance j),
 *   id_last_stuff = num_seg_classes - num_classes, stuff_area_limit in pixels (reference default 4*64*64).
 * pan_2ch uint8 [H,W,3]: channel 0 = category, channel 1 = instance id (enumerate index + 1, 0 for stuff/void), channel 2 = 0.
 * workspace: upsnet_unified_pan_workspace_bytes() bytes of device memory (zeroed by the call). */
size_t upsnet_unified_pan_workspace_bytes(void);
int upsnet_unified_pan_result(void *stream, const int64_t *pan, const int64_t *seg, const int64_t *cls_inds, int num_inst,
                              int height, int width, int id_last_stuff, int num_seg_classes, int stuff_area_limit,
                              void *workspace, unsigned char *pan_2ch);

/* BaseDataset.get_combined_pan_result (upsnet/dataset/base_dataset.py:373-449) for a chunk of images in one call, on the device:
 * the instance masks pasted greedily in merge order, then merged with the semantic map.
 *   images int64 [num_images][8]: height, width, seg (device address of a uint8 [height][width] semantic map), out (device address
 *     of a uint8 [height][width][3] result), first candidate, end of candidates, occupancy word offset (sum of ceil(h * w / 64)
 *     over the earlier images), pixel offset (sum of h * w over the earlier images); every image has 1..2^24 pixels;
 *   cand int32 [n][4]: (class 1..num_classes-1, pixel count > 0, first segment, end of segments), each image's candidates in merge
 *     order (score descending), at most 255 per class; segments int32 [m][2]: column-major pixel ranges [a, b) (p = x * h + y) of
 *     the mask's ones, ascending, none crossing a multiple of 4096; cand / segments may be NULL when there are no candidates.
 * A candidate is accepted iff (float)(remain / area) >= fraction_threshold compared in double (remain = its pixels no earlier
 * accepted candidate claimed); accepted ones are numbered per class from 1 and claim their remaining pixels. out: channel 0 =
 * id_last_stuff + class on claimed pixels, else 255 where seg > id_last_stuff or seg is a stuff label with fewer than
 * stuff_area_limit pixels, else seg; channel 1 = instance number (0 if unclaimed); channel 2 = 0.
 * workspace: upsnet_combined_pan_workspace_bytes(num_images, total_pixels) bytes (total_pixels = sum of h * w), 256-byte aligned.
 * Four launches on `stream` (one memset), no host synchronisation. */
size_t upsnet_combined_pan_workspace_bytes(int num_images, long total_pixels);
int upsnet_combined_pan_result(void *stream, int num_images, const int64_t *images, int max_height, int max_width, long total_pixels,
                               const int *cand, const int *segments, int id_last_stuff, int num_classes, int stuff_area_limit,
                               double fraction_threshold, void *workspace);

/* im_post (upsnet/upsnet_end2end_test.py:95-152) without the full-image pass per detection: for detection d the mask
 * probability of its class (mask_prob [n, C, M, M]; C == 1: class-agnostic) is zero-padded to (M+2)^2, resized (cv2
 * INTER_LINEAR) to the box expanded by (M+2)/M and truncated to int32 (expand_boxes, bbox_transform.py:365-381), thresholded
 * at 0.5 and pasted into an im_height x im_width mask -- of which only the run-length encoding is produced:
 * transitions[d, 0..transition_count[d]) are the column-major pixel indices (x * im_height + y) at which the mask value changes,
 * ascending (the first one starts the first run of ones). pycocotools' counts are the differences of [0, transitions..., H*W].
 * transition_count[d] > cap signals overflow (retry with a larger cap). pred_boxes [n,4] in image coordinates. */
int upsnet_im_post_rle(void *stream, const float *pred_boxes, const float *mask_prob, const int64_t *cls_inds, int num_det,
                       int num_mask_channels, int mask_size, int im_height, int im_width, int cap, unsigned *transitions,
                       int *transition_count);

/* The semantic and panoptic label maps of one image restored to another resolution by a nearest-neighbour gather (the reference's
 * crop + astype('uint8') + cv2.resize(fx = 1 / im_scale, INTER_NEAREST), upsnet/upsnet_end2end_test.py:258-272; also PIL's NEAREST
 * resize in evaluate_ssegs): out[y][x] = (uint8) src[y_ofs[y]][x_ofs[x]], the low byte kept (numpy's astype('uint8') wrap).
 *   sseg, pano int64 [src_height][src_stride] (row stride in elements, src_stride >= src_width); pano may be NULL (then out_pano too);
 *   y_ofs int32 [out_height], x_ofs int32 [out_width]: source row / column of every output row / column (the host builds them;
 *     entries outside the source are clamped to it); out_sseg, out_pano uint8 [out_height][out_width], row-major.
 * Both maps in one launch, no host synchronisation. */
int upsnet_restore_label_maps(void *stream, const int64_t *sseg, const int64_t *pano, long src_stride, int src_height, int src_width,
                              const int *y_ofs, int out_height, const int *x_ofs, int out_width, unsigned char *out_sseg,
                              unsigned char *out_pano);

/* The same gather for one uint8 plane (the panoptic confidence of upsnet_panoptic_fuse_up_conf, which thereby reaches the original
 * image size by the rule of the label maps): out[y][x] = src[y_ofs[y]][x_ofs[x]]; src uint8 [src_height][src_stride], out uint8
 * [out_height][out_width]. One launch, no host synchronisation. */
int upsnet_restore_plane_u8(void *stream, const unsigned char *src, long src_stride, int src_height, int src_width, const int *y_ofs,
                            int out_height, const int *x_ofs, int out_width, unsigned char *out);

/* ============================== Evaluation: panoptic quality and semantic confusion matrix ============================== */

/* BaseDataset.evaluate_panoptic -> _pq_compute_single_core (upsnet/dataset/base_dataset.py:209-330,514-610) for one image, on the
 * device, added into running per-category accumulators:
 *   pred_2ch uint8 [H,W,3] (get_unified_pan_result's output: channel 0 category, 255 = VOID; channel 1 instance);
 *   gt_rgb uint8 [H,W,3] GT panoptic PNG, id = R + 256 G + 65536 B, id 0 = VOID;
 *   segments int64 [num_segments][4] = (id, category_id, iscrowd, area) in segments_info (JSON) order, area as given in the JSON;
 *   cat_known uint8 [256]: non-zero for the categories of the dataset's category table;
 *   tp / fp / fn int64 [256], iou float64 [256]: accumulators indexed by category (added to, never cleared);
 *   status uint64 [1]: the first error, 0 if none; ((image_index + 1) << 8 | category) when a pred category is not in cat_known
 *     (that image then adds nothing, like the reference, which raises KeyError).
 * workspace: upsnet_pq_workspace_bytes(max_gt) bytes (0 for max_gt outside 0..4096), 8-byte aligned, ZEROED ONCE before its first
 * use; every call leaves it zeroed again. num_segments <= max_gt, H * W < 2^31. Three launches on `stream`, no host synchronisation.
 * Ids must be unique and non-zero, categories in 0..254 (the caller validates; the kernels stay in bounds regardless). */
size_t upsnet_pq_workspace_bytes(int max_gt);
int upsnet_pq_accumulate(void *stream, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                         const int64_t *segments, int num_segments, const unsigned char *cat_known, int image_index, int max_gt,
                         void *workspace, int64_t *tp, int64_t *fp, int64_t *fn, double *iou, uint64_t *status);

/* Boundary PQ (Cheng et al., Boundary IoU, CVPR 2021; csrc/pq_boundary.hip): upsnet_pq_accumulate with every pair scored by
 * min(mask IoU, boundary IoU). A pixel of a label map is interior iff the (2 * dilation + 1)^2 window centred on it lies inside the
 * image and holds the pixel's own label throughout; its boundary bit is "not interior" (every pixel when 2 * dilation + 1 exceeds the
 * height or the width). Labels: GT the 24-bit PNG id, pred cat << 8 | inst with all cat == 255 pixels one VOID label. dilation >= 1 is
 * upsnet_amd.dataset.boundary.boundary_dilation(height, width, ratio) on the host; there is no upper limit.
 * upsnet_pan_boundary_map: out_bits uint8 [H,W], bit 0 = GT boundary, bit 1 = pred boundary, every byte written; either map, not both, may
 * be NULL (its bit stays 0). workspace: upsnet_pan_boundary_workspace_bytes(height, width) bytes, no zeroing, no alignment. Two launches
 * (one when the window exceeds the image).
 * upsnet_pq_boundary_accumulate: all other arguments as upsnet_pq_accumulate. workspace: upsnet_pq_boundary_workspace_bytes(max_gt,
 * height, width) bytes (0 for arguments out of range; a workspace sized for a larger image serves a smaller one), 16-byte aligned,
 * ZEROED ONCE before its first use; every call leaves its count areas zeroed again. Five launches on `stream`, no host synchronisation,
 * no allocation. Non-zero return (upsnet_last_error) before anything is launched: null pointers, non-positive sizes, dilation < 1. */
size_t upsnet_pan_boundary_workspace_bytes(int height, int width);
int upsnet_pan_boundary_map(void *stream, int dilation, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                            void *workspace, unsigned char *out_bits);
size_t upsnet_pq_boundary_workspace_bytes(int max_gt, int height, int width);
int upsnet_pq_boundary_accumulate(void *stream, int dilation, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height,
                                  int width, const int64_t *segments, int num_segments, const unsigned char *cat_known, int image_index,
                                  int max_gt, void *workspace, int64_t *tp, int64_t *fp, int64_t *fn, double *iou, uint64_t *status);

/* BaseDataset.get_confusion_matrix (upsnet/dataset/base_dataset.py:806-824) added into confusion int64 [class_num, class_num]:
 * for every pixel with gt_label != ignore_label (ignore_label = -1: no pixel dropped), index = gt * class_num + pred, counted iff
 * index < class_num^2 -- a pred value >= class_num therefore aliases into another cell, as np.bincount does in the reference.
 * gt_label / pred_label uint8 [npix]; class_num in 1..256. */
int upsnet_confusion_accumulate(void *stream, const unsigned char *gt_label, const unsigned char *pred_label, long npix,
                                int class_num, int ignore_label, int64_t *confusion);

/* ============================== Evaluation: COCO box / mask AP (pycocotools COCOeval, default Params) ============================== */

/* COCOeval.evaluate() for ONE image, on the device: computeIoU + evaluateImg (maxDet 100) for every category row, written as one record
 * per detection at rec_*[0 .. num_det) (the caller passes the arrays offset to this image's first record):
 *   rec_score double (the det score), rec_img int (image_index), rec_rk int (row << 8 | rank inside (image, row), score descending,
 *   ties in input order; -1 when the class has no row or the rank is >= 100), rec_match / rec_ign uint64: bit a * 10 + t = matched /
 *   ignored for area range a and IoU threshold t (written only for rec_rk >= 0). npig int64 [num_rows][4] += the non-ignored GTs.
 * Detections: det_score double [num_det], det_cls int64 [num_det] (1-based classes; row = class_to_row[cls] for 0 <= cls < num_classes,
 *   -1 = not scored); bbox: det_xyxy double [num_det][4] (x2 - x1 + 1 = width, as xyxy_to_xywh); segm: either det_box_f32 [num_det][4]
 *   + mask_prob float [num_det][num_mask_channels][mask_size][mask_size] pasted by the im_post rule, or run-lengths det_trans (sorted
 *   column-major change positions, the first starting a run of ones) with det_trans_off int64 [num_det + 1].
 * GT, grouped by row (gt_row_off int [num_rows + 1]), input order inside a row: gt_box double [num_gt][4] xywh (bbox), gt_area double
 *   (the JSON area: area ranges only), gt_crowd int; segm masks: run-lengths (gt_trans, gt_trans_off [num_gt_rle + 1], gt_trans_dst =
 *   the GT index of each) and / or uint8 [H,W] device masks gt_u8[j] (a HOST array of device pointers) for GT gt_u8_dst[j] (host ints).
 * rows_with_gt int [num_rows_with_gt]: the rows with at least one GT. params double [18]: min(iouThr, 1 - 1e-10) for the 10 thresholds,
 *   then (lo, hi) of the 4 area ranges. workspace: upsnet_det_eval_image_workspace_bytes(...) bytes, 256-byte aligned; no zeroing.
 * H * W < 2^31; scores must not be NaN. Launches on `stream` only, no host synchronisation. */
size_t upsnet_det_eval_image_workspace_bytes(int num_det, int num_rows, int num_gt, int height, int width, int segm);
int upsnet_det_eval_image(void *stream, int segm, int height, int width, int num_rows, int num_det, const double *det_xyxy,
                          const double *det_score, const int64_t *det_cls, const int *class_to_row, int num_classes,
                          const float *det_box_f32, const float *mask_prob, int num_mask_channels, int mask_size,
                          const int *det_trans, const int64_t *det_trans_off, int num_gt, const int *gt_row_off,
                          const double *gt_box, const double *gt_area, const int *gt_crowd, const int *gt_trans,
                          const int64_t *gt_trans_off, const int *gt_trans_dst, int num_gt_rle, const unsigned char *const *gt_u8,
                          const int *gt_u8_dst, int num_gt_u8, const int *rows_with_gt, int num_rows_with_gt,
                          const double *params, int image_index, void *workspace, double *rec_score, int *rec_img, int *rec_rk,
                          uint64_t *rec_match, uint64_t *rec_ign, int64_t *npig);

/* COCOeval.accumulate() over num_records records of upsnet_det_eval_image: img_ord int [number of images]: the position of image_index
 * in ascending image_id order; rec_thrs double [101] (recThrs); npig as accumulated. Outputs (fully written): precision / scores double
 * [10][101][num_rows][4][3], recall double [10][num_rows][4][3], -1 where npig == 0. workspace:
 * upsnet_det_eval_accumulate_workspace_bytes(num_records, num_rows) bytes, 256-byte aligned; no zeroing. */
size_t upsnet_det_eval_accumulate_workspace_bytes(long num_records, int num_rows);
int upsnet_det_eval_accumulate(void *stream, long num_records, const double *rec_score, const int *rec_img, const int *rec_rk,
                               const uint64_t *rec_match, const uint64_t *rec_ign, const int *img_ord, int num_rows,
                               const int64_t *npig, const double *rec_thrs, void *workspace, double *precision, double *recall,
                               double *scores);

/* Boundary AP (the Boundary IoU API's COCOeval with iouType 'boundary', Cheng et al. 2021): upsnet_det_eval_image's mask evaluation with
 * IoU = min(rleIou of the masks, rleIou of their boundaries), boundary = mask & ~erode(mask), the erosion `dilation` (>= 1) rounds of a 3x3
 * square on the zero-padded mask, i.e. the AND over the (2 * dilation + 1)^2 window with everything outside the image read as 0
 * (mask_to_boundary; dilation = upsnet_amd.dataset.boundary.boundary_dilation(height, width, ratio) on the host). Crowd GTs get a
 * boundary like any other; a detection's area stays its mask's. All other arguments, the records and npig as upsnet_det_eval_image with
 * segm = 1 (no det_xyxy / gt_box). workspace: upsnet_det_eval_boundary_image_workspace_bytes(...) bytes, 256-byte aligned; no zeroing.
 * upsnet_boundary_dilation_fits: 1 when the erosion window of `dilation` fits the kernel's tile on this image size (always when
 * 2 * dilation + 1 exceeds the height or the width, else up to dilation 3056); the entry points refuse a dilation that does not. */
size_t upsnet_det_eval_boundary_image_workspace_bytes(int num_det, int num_rows, int num_gt, int height, int width);
int upsnet_det_eval_boundary_image(void *stream, int dilation, int height, int width, int num_rows, int num_det,
                                   const double *det_score, const int64_t *det_cls, const int *class_to_row, int num_classes,
                                   const float *det_box_f32, const float *mask_prob, int num_mask_channels, int mask_size,
                                   const int *det_trans, const int64_t *det_trans_off, int num_gt, const int *gt_row_off,
                                   const double *gt_area, const int *gt_crowd, const int *gt_trans,
                                   const int64_t *gt_trans_off, const int *gt_trans_dst, int num_gt_rle,
                                   const unsigned char *const *gt_u8, const int *gt_u8_dst, int num_gt_u8, const int *rows_with_gt,
                                   int num_rows_with_gt, const double *params, int image_index, void *workspace, double *rec_score,
                                   int *rec_img, int *rec_rk, uint64_t *rec_match, uint64_t *rec_ign, int64_t *npig);
int upsnet_boundary_dilation_fits(int height, int width, int dilation);

/* mask_to_boundary of num_masks masks of one size with the evaluator's kernel: either masks_u8 uint8 [num_masks][H][W] (non-zero = set)
 * or run-lengths trans (ascending column-major change positions, the first starting a run of ones) with trans_off int64
 * [num_masks + 1]. Outputs (fully written): boundary_u8 uint8 [num_masks][H][W] of 0 / 1, boundary_area int [num_masks] (its pixels).
 * workspace: upsnet_boundary_masks_workspace_bytes(num_masks, height, width) bytes, 256-byte aligned; no zeroing. H * W < 2^31,
 * num_masks <= 65535. Launches on `stream` only, no host synchronisation. */
size_t upsnet_boundary_masks_workspace_bytes(int num_masks, int height, int width);
int upsnet_boundary_masks(void *stream, int dilation, int height, int width, int num_masks, const unsigned char *masks_u8,
                          const int *trans, const int64_t *trans_off, void *workspace, unsigned char *boundary_u8, int *boundary_area);

/* Polygon GT -> run-length masks for upsnet_det_eval_image (gt_trans / gt_trans_off), all polygon objects of ONE image: pycocotools'
 * rleFrPoly (frPyObjects of a polygon list) and merge (union) restated from the published algorithm (csrc/poly_raster.hip).
 *   vertices double [total_vertices][2] (x, y) on the device; poly_off int [num_poly + 1]: the first vertex of each polygon;
 *   obj_off int [num_obj + 1]: the first polygon of each object. Both tables are given twice, on the HOST (validated here: start at 0,
 *   monotone, obj_off[num_obj] = num_poly) and as device copies (*_dev) that the kernels read.
 *   total_points: the sum over all edges (every vertex starts one, the last vertex of a polygon back to the first) of
 *   max(|dX|, |dY|) + 1 with X = (int)(5 * x + .5), Y likewise -- an exact upper bound of the positions emitted; at most 2^24.
 *   The caller guarantees finite coordinates with |5 * c| < 2^30 (the vertices are device data and are not inspected).
 * Outputs on the device: trans int [total_points] (the first trans_off[num_obj] entries are written: per object the ascending
 *   column-major positions x * height + y in [0, H * W) where the mask changes, the first starting a run of ones), trans_off int64
 *   [num_obj + 1] (fully written). An object without polygons, or whose polygons emit nothing, has an empty list.
 * workspace: upsnet_poly_raster_workspace_bytes(total_vertices, total_points) bytes (0 = arguments out of range), 256-byte aligned; no
 * zeroing. H * W < 2^31. Launches on `stream` only, no host synchronisation, no allocation; the result does not depend on how objects
 * are grouped into calls. */
size_t upsnet_poly_raster_workspace_bytes(long total_vertices, long total_points);
int upsnet_poly_raster(void *stream, const double *vertices, const int *poly_off, const int *obj_off, const int *poly_off_dev,
                       const int *obj_off_dev, int num_poly, int num_obj, long total_points, int height, int width, void *workspace,
                       int *trans, int64_t *trans_off);

/* ============================== Evaluation: RPN proposal recall (Detectron's AR, evaluate_box_proposals) ============================== */

/* BaseDataset.evaluate_box_proposals (upsnet/dataset/base_dataset.py:723-805), the greedy matching of each (image, area, limit) problem,
 * on the device: repeatedly take the alive GT column with the largest max IoU over the alive proposal rows (the first column among
 * equal maxima), record that IoU, delete the column and its argmax row (the first row among equal IoUs). IoU = bbox_overlaps_c of
 * upsnet/bbox/bbox.pyx in fp32, same operation order (bit-identical).
 *   problems int64 [num_problems][6]: proposal offset (rows of `proposals`), P (proposals of the problem, in rank order), GT offset
 *     (rows of `gt_boxes`), G (0..max_gt), output offset (floats of `out`), workspace word offset (uint32 words; the problems' ranges
 *     of ceil(P / 32) words are disjoint and inside the workspace);
 *   proposals / gt_boxes float [.][4] x1 y1 x2 y2, 16-byte aligned, finite.
 * out float [G] per problem at its offset (fully written): the IoU recorded at step j (j < min(P, G)), then zeros. A row with P < 0,
 * G < 0 or G > 4096 breaks the contract: the kernel skips it (nothing read or written for it).
 * max_gt <= 4096; total_proposals = sum of P over the problems (< 2^31). workspace: upsnet_proposal_recall_workspace_bytes(num_problems,
 * total_proposals) bytes, 256-byte aligned; no zeroing. One launch on `stream`, no host synchronisation. */
size_t upsnet_proposal_recall_workspace_bytes(int num_problems, long total_proposals);
int upsnet_proposal_recall(void *stream, int num_problems, const int64_t *problems, const float *proposals, const float *gt_boxes,
                           int max_gt, long total_proposals, void *workspace, float *out);

/* ============================== Evaluation: Cityscapes instance-level AP (the devkit's region AP) ============================== */

/* The per-image part of the Cityscapes devkit's evalInstanceLevelSemanticLabeling (default arguments; the rules are restated in
 * dataset/cityscapes_eval.py and DESIGN 4.10), csrc/cs_inst_eval.hip. All on `stream`, no host synchronisation, no allocation.
 *   gt_ids uint16 [height][width]: the gtFine_instanceIds map on the device; height * width <= 2^30.
 *   pred_cls int [num_preds] (1..8 = person rider car truck bus train motorcycle bicycle), pred_scores float [num_preds] (not NaN;
 *   device data, not inspected). Masks either as run lengths -- trans int [trans_off[num_preds]], trans_off int [num_preds + 1]: per
 *   prediction the ascending column-major positions x * height + y in [0, H * W) where the mask changes, the first starting a run of
 *   ones; masks = NULL -- or dense, masks uint8 [num_preds][height][width] (non-zero = inside; trans = trans_off = NULL).
 *   walk_strided = 0: the run lists are walked over a transposed copy of the map written to gt_t (uint16 [width][height]);
 *   walk_strided = 1: over the row-major map itself (gt_t unused). Same counts either way.
 *   thresholds: num_thr (1..16) doubles on the HOST, each in [0.5, 1): above 0.5 a prediction overlaps at most one region.
 * Outputs on the device:
 *   counts int [upsnet_cs_inst_counts_ints(num_preds)] (zeroed here): per prediction 1003 ints = area | intersection with void pixels |
 *     intersection with slot 0..1000 of its class (slot 0 = the group region, raw value = label id; slot 1 + k = raw value 1000 * label
 *     id + k), then int [8][1001]: the pixel count of every slot of every class;
 *   rec_score float [num_preds] (a copy), rec_cls uint8 [num_preds] (the class; 0 = a prediction of no pixels, dropped), rec_code uint8
 *     [num_preds][num_thr]: 1 = the entry (1, score), 2 = the entry (0, score), 0 = no entry (ignored, or matched to a group / small
 *     region only); rows of a class outside 1..8 are not written;
 *   state int64 [upsnet_cs_inst_state_words()], running sums the caller zeroes once: hard false negatives [8][16] (class, threshold) |
 *     images with a valid GT region [8] | predictions of non-zero area [8].
 * workspace: upsnet_cs_inst_workspace_bytes(num_preds) bytes, 8-byte aligned, no zeroing. num_preds = 0 (all prediction pointers may be
 * NULL) still counts the image's GT. Both size functions return 0 for num_preds outside 0..65535. */
size_t upsnet_cs_inst_counts_ints(int num_preds);
size_t upsnet_cs_inst_workspace_bytes(int num_preds);
int upsnet_cs_inst_state_words(void);
int upsnet_cs_inst_image(void *stream, const uint16_t *gt_ids, int height, int width, int num_preds, const int *pred_cls,
                         const float *pred_scores, const int *trans, const int *trans_off, const unsigned char *masks, int walk_strided,
                         uint16_t *gt_t, const double *thresholds, int num_thr, int *counts, void *workspace, float *rec_score,
                         unsigned char *rec_cls, unsigned char *rec_code, int64_t *state);

/* ============================== Evaluation: Cityscapes pixel-level IoU / iIoU ============================== */

/* The per-image part of the Cityscapes devkit's evalPixelLevelSemanticLabeling (the rules are restated in
 * dataset/cityscapes_pixel_eval.py and DESIGN 4.12), csrc/cs_pixel_eval.hip. All on `stream`, no host synchronisation, no allocation.
 *   gt_labels uint8 [height][width]: the gtFine_labelIds map; gt_ids uint16 [height][width]: the gtFine_instanceIds map, or NULL
 *   (confusion matrix only: inst, wsum and avg_class_size are then unused and may be NULL); pred uint8 [height][width];
 *   lut uint8 [256] on the device: label id of every prediction value, anything above 33 = "not a label". height * width <= 2^30.
 *   avg_class_size: 8 positive doubles on the HOST (person rider car truck bus train motorcycle bicycle).
 * Outputs on the device:
 *   conf int64 [34][34], running sums the caller zeroes once: conf[gt label][pred label], every pixel counted;
 *   inst int [upsnet_cs_pixel_inst_ints()] = [8][1000][3] (zeroed here): for the instance of raw value 1000 * label + k > 1000 of
 *     class c: pixels | pixels with pred == label | pixels whose pred is an evaluated label of the label's category;
 *   wsum double [10][4], running sums the caller zeroes once: rows = the 8 classes, human, vehicle; columns = tp | tpWeighted | fn |
 *     fnWeighted, each instance added in ascending raw value with weight avg_class_size / pixels (float64, the devkit's order);
 *   bad int [2], zeroed by the caller: pixels whose prediction is not a label (added to [0]) or whose ground-truth label is above 33
 *     ([1]); such pixels enter no other count. */
size_t upsnet_cs_pixel_inst_ints(void);
int upsnet_cs_pixel_image(void *stream, const unsigned char *gt_labels, const uint16_t *gt_ids, const unsigned char *pred,
                          const unsigned char *lut, int height, int width, const double *avg_class_size, int64_t *conf, int *inst,
                          double *wsum, int *bad);

/* ============================== COCO panoptic format: write and read back panoptic predictions ============================== */

/* _converter_2ch_single_core (upsnet/dataset/base_dataset.py:463-511, without vis_panoptic) for one image, on the device:
 *   pred_2ch uint8 [H,W,3] (channel 0 category, 255 = VOID; channel 1 instance); a segment is a key = ch0 << 8 | ch1 with ch0 != 255;
 *   cat_table int [256]: -1 for a category that is not in the dataset's table, else R | G << 8 | B << 16 | isthing << 24;
 *   rgb uint8 [H,W,3] (out): the segment's colour, id = R + 256 G + 65536 B; VOID pixels (0,0,0);
 *   table int [upsnet_pan_format_table_ints()] (out): [0] = number of segments n, [1] = error (0 none, 1 = a segment's category is
 *     not in cat_table, 2 = no free colour left around a category's base), [2] = the category of the error (the lowest for error 1),
 *     [3..7] = 0, then n rows of 8 ints in ascending key (np.unique's order): key, area, x_min, y_min, x_max, y_max, id, ordinal of
 *     the segment within its category. Rows past n are not written. The colour rule is documented in csrc/pan_format.hip and
 *     DESIGN.md section 4.11; the same map and table give the same bytes on every run (integer atomics only).
 * workspace: upsnet_pan_format_workspace_bytes() bytes, 4-byte aligned, ZEROED ONCE before its first use; every call leaves it
 * zeroed again except for its colour table. H * W < 2^31. Three launches on `stream`, no host synchronisation. */
size_t upsnet_pan_format_workspace_bytes(void);
size_t upsnet_pan_format_table_ints(void);
int upsnet_pan_format(void *stream, const unsigned char *pred_2ch, int height, int width, const int *cat_table, void *workspace,
                      unsigned char *rgb, int *table);

/* Panoptic PNG -> 2-channel map: rgb uint8 [H,W,3] (id = R + 256 G + 65536 B); table int [num_segments][3] = (id, category, instance
 * slot 0..255), SORTED BY ID, ids unique in 1..2^24-1 (the caller validates; the kernels stay in bounds regardless);
 * out_2ch uint8 [H,W,3] = (category, slot, 0), id 0 and ids missing from the table -> (255, 0, 0); counts int [num_segments], zeroed by
 * the caller: pixels per table row (added). status uint64 [2], zeroed once by the caller, kept across images: [0] = 2^62 -
 * ((image_index + 1) << 24 | id) for the smallest non-zero id of the earliest image that is in the PNG and not in the table, [1] =
 * the same for a table row without a pixel; 0 = none. num_segments in 0..65280 (up to 4096 the table is searched in LDS). */
int upsnet_pan_relabel(void *stream, const unsigned char *rgb, int height, int width, const int *table, int num_segments,
                       int image_index, unsigned char *out_2ch, int *counts, uint64_t *status);

/* ============================== Evaluation ground truth from the raw Cityscapes download ============================== */

/* One gtFine_instanceIds map -> the labelTrainIds map, the panoptic PNG content with its segment table, and the run-length
 * transitions of every instance mask (csrc/gt_prepare.hip; the rules are restated in dataset/prepare.py and DESIGN 4.14).
 *   ids int [height][width]: raw value v in 0..255 (label v) or 1000..65535 (label v / 1000, at most 65); label_ids uint8
 *   [height][width] or NULL: the gtFine_labelIds map, only cross-checked; train_id, has_instances, thing_row: int [256] each on the device, indexed by label:
 *   train id (255 = ignored in evaluation), hasInstances (0 / 1), row 0..7 of a thing class or -1 (only for labels that are not ignored).
 * Outputs on the device:
 *   train_map uint8 [height][width]: the label's train id; rgb uint8 [height][width][3]: (v % 256, v / 256 % 256, v / 65536), and
 *     (0,0,0) where the label is ignored; every byte of both is written;
 *   table int [seg_capacity][9]: the distinct v whose label is not ignored, ascending: v, label, train id, iscrowd (v < 1000 and the
 *     label has instances), area, x_min, y_min, x_max, y_max; rows past the count are not written;
 *   instances = the segments with v >= 1000 and a thing row, ascending v; trans_off int [seg_capacity + 1]: [0 .. instances] are
 *     written; trans int [trans_capacity]: for instance j, trans[trans_off[j] .. trans_off[j + 1]) are the ascending column-major
 *     positions x * height + y at which (ids == v) changes (0 before the first pixel): the lists dataset/rle.py turns into RLE counts;
 *   status int [8] (zeroed here): [0] segments, [1] instances, [2] transitions (the true counts, also beyond the capacities),
 *     [3] flags: 1 = more segments than seg_capacity (no instance list is made, [2] = 0), 2 = more transitions than trans_capacity
 *     (trans is not written), 4 = a value that encodes no label (negative, 256..999 or beyond 65535: treated as ignored, no table
 *     is indexed with it, the outputs are not to be used); [4] pixels of label_ids that differ from the label of ids (a value
 *     without a label differs); [5..7] = 0. Nothing is written out of bounds in either case, and the next call on the workspace is unaffected.
 * workspace: upsnet_gt_prepare_workspace_bytes(seg_capacity) bytes (0 for a capacity outside 1..65536), 4-byte aligned, ZEROED ONCE
 * before its first use; every call leaves it as it needs it. height, width <= 32768, height * width < 2^30. Six launches on `stream`,
 * integer atomics only: the same input gives the same bytes on every run. No host synchronisation, no allocation. */
size_t upsnet_gt_prepare_workspace_bytes(int seg_capacity);
int upsnet_gt_prepare(void *stream, const int *ids, const unsigned char *label_ids, int height, int width, const int *train_id,
                      const int *has_instances, const int *thing_row, int seg_capacity, int trans_capacity, void *workspace,
                      unsigned char *train_map, unsigned char *rgb, int *table, int *trans_off, int *trans, int *status);

/* ============================== Detection visualisations (config.test.vis_mask) ============================== */

/* One image of the reference's vis_all_mask (upsnet/dataset/base_dataset.py:826-896) by the integer drawing rule of DESIGN.md section
 * 4.13 (restated in the header of csrc/vis_render.hip): box ring, mask fill and contour per detection in order, then the labels.
 *   image uint8 [height][width][3] RGB; out the same shape (every byte written, each once; must not overlap image);
 *   the num_dets detections in drawing order: boxes float [n][4] (x1 y1 x2 y2), colours uint8 [n][3] (RGB of the mask fill), labels
 *   uint8 [n][upsnet_vis_max_label()] of which the first label_len[n] bytes are drawn; masks as the evaluators pass them: trans int
 *   [num_trans], the ascending column-major change positions x * height + y of all masks one after the other, trans_off int [n + 1]
 *   the first position of each list (trans_off[n] = num_trans). Lists that are not ascending or leave the image draw a wrong picture;
 *   the kernels stay inside their arrays regardless.
 * Limits (error code, nothing clamped): sides 1..32768, height * width <= 2^28, num_dets 0..upsnet_vis_max_detections() (256), a
 * label_len above upsnet_vis_max_label() (32) is the caller's to refuse (the kernel reads no further than 32 bytes).
 * workspace: upsnet_vis_workspace_bytes(num_dets, height, width) bytes (0 for sizes beyond the limits), 4-byte aligned; NO zeroing is
 * asked of the caller and nothing is kept between calls. Four launches on `stream`, no host synchronisation, no allocation, no atomics
 * on the canvas: the same input gives the same bytes on every run.
 * upsnet_vis_font: the 95 cells (characters 32..126) of the label font into cells uint8 [95][8] on the HOST: one byte per cell row,
 * bit 4 = the leftmost of 5 dots, the eighth row empty. */
int upsnet_vis_max_detections(void);
int upsnet_vis_max_label(void);
size_t upsnet_vis_workspace_bytes(int num_dets, int height, int width);
int upsnet_vis_font(unsigned char *cells);
int upsnet_vis_render(void *stream, const unsigned char *image, int height, int width, int num_dets, const float *boxes,
                      const unsigned char *colours, const unsigned char *labels, const int *label_len, const int *trans,
                      const int *trans_off, int num_trans, void *workspace, unsigned char *out);

/* ============================== Panoptic visualisations (vis_panoptic: flat and overlay) ============================== */

/* One panoptic prediction as a picture, by the integer drawing rule of DESIGN.md section 4.20 (restated in the header of
 * csrc/pan_vis.hip). mode 0 (flat): the reference's vis_panoptic picture (upsnet/dataset/base_dataset.py:463-511): every
 * pixel in its category colour, white two-pixel contours around the thing instances. mode 1 (overlay): the photograph with
 * every segment in its own colour at 1/2, the segment borders in white at 1/2 and the category names at the segments' centroids.
 *   pred_2ch uint8 [height][width][3] (channel 0 category, 255 = VOID; channel 1 instance), cat_table int [256] as upsnet_pan_format
 *   takes it; out uint8 [height][width][3] (every byte written, each once; must overlap no input);
 *   info int [2] (out): [0] = segments of area >= label_min_area, [1] = labels drawn (the first upsnet_pan_vis_max_labels() = 256 of
 *   them in ascending key); both 0 in flat mode.
 * Overlay runs on the same stream AFTER upsnet_pan_format on the same map: id_rgb uint8 [height][width][3] and seg_table are that
 * call's `rgb` and `table`; image uint8 [height][width][3] RGB; names uint8 [256][32] and name_len int [256]: the label of every
 * category (a name_len outside 0..32 is taken as the nearer bound; bytes outside 32..126 draw as '?'). Flat reads none of id_rgb,
 * seg_table, image, names, name_len (they may be NULL) and ignores label_min_area's value.
 * Error code before anything is launched: a null pointer, another mode, sides outside 1..32768, height * width > 2^28, a negative
 * label_min_area. A seg_table that does not belong to the map draws a wrong picture; the kernels stay inside their arrays regardless.
 * workspace: upsnet_pan_vis_workspace_bytes() bytes, 16-byte aligned; its first upsnet_pan_vis_workspace_zeroed_bytes() bytes ZEROED
 * ONCE before the first use, every call leaves them zeroed again; the rest needs no zeroing. Overlay: three launches, flat: one; no
 * host synchronisation, no allocation, no atomics on the picture: the same input gives the same bytes on every run. */
size_t upsnet_pan_vis_workspace_bytes(void);
size_t upsnet_pan_vis_workspace_zeroed_bytes(void);
int upsnet_pan_vis_max_labels(void);
int upsnet_pan_vis(void *stream, int mode, const unsigned char *pred_2ch, const unsigned char *id_rgb, const int *seg_table,
                   const unsigned char *image, int height, int width, const int *cat_table, const unsigned char *names,
                   const int *name_len, int label_min_area, void *workspace, unsigned char *out, int *info);

/* ============================== GroupNorm heads (with_norm = 'group_norm') ============================== */

/* nn.GroupNorm(32, C) with a fused epilogue (csrc/group_norm.hip):
 *   out = relu?( (x - mean_g) * rstd_g * gamma_c + beta_c  [+ residual | + nearest x2 upsampled residual] ),  rstd = 1 / sqrt(var + eps),
 * mean / biased variance per (sample, group) over C / 32 channels x height x width pixels.
 * Preconditions of all forms: x, out (and residual) fp32, NHWC-dense (channels-last), 16-byte aligned; gamma, beta fp32 [C], 16-byte
 * aligned, read in place; C % 128 == 0 and C <= 1024 (a lane owns 4 channels of one group; every head width of the model: 128, 256,
 * 1024) -- any other C is an error code, nothing runs. eps >= 0. Empty maps (batch, height or width 0) are skipped.
 * Sums are fp64 from the first add, combined in an order fixed by the shape of one sample: the value of a sample does not depend on
 * the batch size, on the other maps of the launch or on the run (no atomics); var is never formed as E[x^2] - mean^2 in fp32.
 *
 * upsnet_group_norm_nhwc_f32: 1..5 maps x[i] [batch[i], height[i], width[i], C] sharing gamma / beta, two launches (partials per chunk
 * of upsnet_group_norm_chunk_pixels() pixels into `workspace`, then recombine + apply); bit-identical to one call per map.
 *   residual: NULL, or one pointer per map (entries may be NULL) together with res_height / res_width, the residual's own size:
 *   [batch, height, width, C] (residual_up = 0) or [batch, height / 2, width / 2, C] with even height, width (residual_up = 1: read
 *   through a nearest x2 upsampling); any other size is an error.
 *   out[i] may alias x[i] or a same-size residual[i], not an upsampled one; nothing may alias the workspace.
 *   workspace: upsnet_group_norm_workspace_bytes(nseg, batch, height, width) bytes (0 for invalid arguments), 16-byte aligned,
 *   caller-allocated, no zeroing needed, nothing kept between calls.
 * upsnet_group_norm_small_nhwc_f32: samples of height * width <= upsnet_group_norm_chunk_pixels() pixels (ROI maps; fc6 rows as
 * height = width = 1), one launch, one workgroup (rows: half a wave) per sample, no workspace, no residual; out may alias x. For
 * height * width > 1 bit-identical to upsnet_group_norm_nhwc_f32 on the same sample. */
int upsnet_group_norm_chunk_pixels(void);
size_t upsnet_group_norm_workspace_bytes(int nseg, const int batch[], const int height[], const int width[]);
int upsnet_group_norm_nhwc_f32(void *stream, int nseg, const float *const x[], float *const out[], const int batch[],
                               const int height[], const int width[], int C, const float *gamma, const float *beta, float eps,
                               int relu, const float *const residual[], const int res_height[], const int res_width[],
                               int residual_up, void *workspace);
int upsnet_group_norm_small_nhwc_f32(void *stream, const float *x, float *out, int batch, int height, int width, int C,
                                     const float *gamma, const float *beta, float eps, int relu);

/* ============================== Cityscapes instance predictions in benchmark format ============================== */

/* The mask planes of the Cityscapes instance-level prediction files (dataset/cityscapes_inst_format.py),
 * csrc/cs_inst_format.hip: run lists in the form upsnet_cs_inst_image takes -- trans int [trans_off[num_masks]], trans_off int
 * [num_masks + 1], per mask the NON-DECREASING column-major positions x * height + y in [0, H * W) where the mask changes, the first
 * starting a run of ones; equal positions cancel (a run of no pixels) -- expanded row-major on `stream`, no host synchronisation, no
 * allocation, no workspace. The lists are device data and are not inspected: the caller has checked them.
 *   bits = 8: out uint8 [num_masks][height][width], 0 or 255.
 *   bits = 1: out uint8 [num_masks][height][(width + 7) / 8], the row layout of a PNG of bit depth 1: the leftmost pixel of a byte in
 *             its most significant bit, the bits past `width` zero.
 * Every byte of `out` is written (it may be uninitialised), nothing outside it. height * width <= 2^30. num_masks = 0 launches
 * nothing (all pointers may be NULL). */
int upsnet_cs_inst_expand(void *stream, const int *trans, const int *trans_off, int num_masks, int height, int width, int bits,
                          unsigned char *out);

/* ============================== Test-time augmentation: the merge step ============================== */

/* Multi-scale / flip test-time augmentation, csrc/tta.hip. An augmentation a has im_info (Hr_a, Wr_a, s_a); q_a = s_a / s_0 and
 * r_a = s_0 / s_a (float32 divisions made by the caller; augmentation 0 is the base). All arithmetic is float32 in the order DESIGN
 * 4.18 writes it. The geometry arrays (sizes, q / r, resized widths Wr_a as floats, flip flags) are HOST arrays of num_aug entries and
 * travel by value with the launch; 1 <= num_aug <= 8. Outputs are caller-allocated; nothing is synchronised or allocated; every index
 * is clamped to its array.
 *
 * upsnet_tta_seg_merge: maps[a] channels-last [map_h[a]][map_w[a]][num_seg] semantic scores, cell = 4 (quarter-resolution score map)
 *   or 1 (full resolution). out [height][width][num_seg] (the base map's shape):
 *   out = (((sample_0 + sample_1) + ...) + sample_{A-1}) / A, sample_a the bilinear sample (half-pixel centres, clamped to the map) of
 *   maps[a] at ((y + 0.5) q_a - 0.5, (x + 0.5) q_a - 0.5), or for a flipped augmentation at column (Wr_a / cell - (x + 0.5) q_a) - 0.5.
 *   One launch, one store per element; 16-byte accesses when num_seg % 4 == 0 and every base is 16-byte aligned, scalar otherwise. */
int upsnet_tta_seg_merge(void *stream, int num_aug, const float *const maps[], const int map_h[], const int map_w[], const float q[],
                         const float resized_w[], const int flip[], int cell, int num_seg, int height, int width, float *out);

/* upsnet_tta_roi_union: per augmentation rois[a] [capacity,5], delta[a] [capacity,delta_dim], prob[a] [capacity,num_classes] and the
 *   DEVICE count num_rois_dev[a] (int32, clamped to 0..capacity). The valid rows of augmentation a, in their order, go to rows
 *   sum_{b<a} n_b ... of rois_out [num_aug*capacity,5], delta_out, prob_out; *num_out = sum n_a; rows past it are zero. Flipped:
 *   x1f = (Wr_a - 1) - x2, x2f = (Wr_a - 1) - x1 and every dx (delta column 4c) negated. Then x1' = r x1, y1' = r y1,
 *   x2' = r x2 + (r - 1), y2' = r y2 + (r - 1). The prefix over the counts is computed in the kernel: no host read.
 *   num_aug * capacity <= 8192 (the capacity of upsnet_mask_roi); delta_dim % 4 == 0. */
int upsnet_tta_roi_union(void *stream, int num_aug, const float *const rois[], const float *const delta[], const float *const prob[],
                         const int *const num_rois_dev[], const float r[], const float resized_w[], const int flip[], int capacity,
                         int delta_dim, int num_classes, float *rois_out, float *delta_out, float *prob_out, int *num_out);

/* upsnet_tta_boxes_to_aug: boxes [num_boxes,5] of the base frame -> boxes_out [num_aug][num_boxes][5], the inverse rule:
 *   x1' = q x1, y1' = q y1, x2' = q x2 + (q - 1), y2' = q y2 + (q - 1), then the flip. Column 0 is copied. num_boxes = 0 launches
 *   nothing. */
int upsnet_tta_boxes_to_aug(void *stream, int num_aug, const float q[], const float resized_w[], const int flip[], const float *boxes,
                            int num_boxes, float *boxes_out);

/* upsnet_tta_mask_merge: logits[a] and out share one dense layout, [num_rois][num_classes][ms][ms] (nhwc = 0) or
 *   [num_rois][ms][ms][num_classes] (nhwc = 1): out = (((L_0 + L_1) + ...) + L_{A-1}) / A, a flipped augmentation read at column
 *   ms - 1 - x. num_rois = 0 launches nothing. */
int upsnet_tta_mask_merge(void *stream, int num_aug, const float *const logits[], const int flip[], int num_rois, int num_classes,
                          int mask_size, int nhwc, float *out);

/* ============================== Box voting ============================== */

/* Score-weighted box voting on the output of upsnet_mask_roi(_ex) (Detectron's TEST.BBOX_VOTE, `ID` scoring; the reference has none).
 * Inputs: the selection's own rois [num_rois,5], bbox_delta [num_rois,4*num_classes], cls_prob [num_rois,num_classes], the optional
 * DEVICE row count num_rois_dev (clamped to 0..num_rois; NULL: num_rois), im_info, clip_boxes and reg_weights_host; its outputs boxes
 * [cap,5], cls [cap] int64 and the DEVICE count num. voted [cap,5] is caller-allocated and must not overlap boxes.
 *   For k < max(*num, 0) (clamped to cap), c = cls[k] (clamped to 0..num_classes-1), b = boxes[k,1:5]: row r < n is a voter when
 *   cls_prob[r,c] > vote_score_thresh and iou(b, d_r) >= vote_iou_thresh, d_r the class-c decode (+ clip) of row r exactly as the
 *   selection builds its candidates, iou the "+1" IoU; a NaN IoU is no voter. Five fp32 sums S_w = sum w_r, S_i = sum w_r * d_r[i],
 *   w_r = cls_prob[r,c], each term one rounded multiply: partial j (0..63) starts at +0 and adds the voters with r % 64 == j in
 *   ascending r; then for s = 32,16,8,4,2,1: p[j] = p[j] + p[j+s] (j < s); the sum is p[0].
 *   S_w > 0: voted[k,1+i] = S_i / S_w, with clip_boxes clamped again to [0, im_w-1] / [0, im_h-1]; otherwise voted[k,1:5] = b.
 *   voted[k,0] = boxes[k,0].
 *   Rows max(*num, 0) <= k < cap are a bit copy of boxes[k] (a negative *num, the selection's overflow marker, copies every row).
 * One launch; nothing is synchronised or allocated. Refused before any launch: a null pointer, num_rois <= 0, num_classes < 2,
 * cap < 0, vote_iou_thresh NaN or <= 0. cap = 0 launches nothing (boxes / cls / voted may be NULL). */
int upsnet_box_vote(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                    const int *num_rois_dev, int num_classes, const float *im_info, int clip_boxes, const float reg_weights_host[4],
                    float vote_score_thresh, float vote_iou_thresh, const float *boxes, const int64_t *cls, const int *num, int cap,
                    float *voted);

/* ============================== Soft detection selection ============================== */

/* upsnet_mask_roi_ex, class-wise, with soft-NMS in place of the hard NMS (Detectron's TEST.SOFT_NMS; the reference's own call sites,
 * bbox_transform.py:271-288, are unreachable). Inputs and outputs as upsnet_mask_roi_ex with class_agnostic = 0:
 * cap = upsnet_mask_roi_capacity(num_rois, num_classes, 0); num_rois_dev is clamped to 0..num_rois.
 *   Per class c = 1..C-1: the candidates are the rows r < n with cls_prob[r,c] > score_thresh, ascending r, box = the class-c decode
 *   (+ clip) of row r, score = cls_prob[r,c]; on that list cpu_soft_nms(dets, sigma, Nt = nms_thresh, threshold = floor, method)
 *   (cpu_nms.pyx:91-196, bit-identical; method 0 hard, 1 linear, 2 gaussian). The class's result is rows 0..N'-1 of the returned
 *   array in that order: box, DECAYED score, source row. The flat list in (class ascending, soft-NMS order) then goes through the
 *   top-max_det rule of upsnet_mask_roi on the decayed scores (max_det > 0 and more than max_det rows: keep score >= the max_det-th
 *   largest, order preserved), the dummy row when nothing survives and the zero rows up to max(max_det, 256). Of the four outputs
 *   the rows below max(|*num_out|, min(cap, max(max_det, 256))) are defined -- the selection, the dummy row, zero rows --, the rows
 *   from there on are unspecified (upsnet_mask_roi_ex's sentence about rows >= *num_out holds from that row on only).
 *   A class's state is LDS-resident: it holds at most 4096 candidates. A class with more keeps its first 4096 and the count comes
 *   out NEGATIVE (the overflow convention of upsnet_mask_roi); with num_rois <= 4096 this cannot happen.
 * Two launches (one workgroup per class, then the finalize); nothing is synchronised or allocated. Refused before any launch: a null
 * pointer, num_rois < 1 or > 8192, num_classes < 2, method outside 0..2, sigma not > 0 with method 2, a NaN nms_thresh or floor. */
size_t upsnet_mask_roi_soft_workspace_bytes(int num_rois, int num_classes);
int upsnet_mask_roi_soft(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                         const int *num_rois_dev, int num_classes, const float *im_info, int clip_boxes, float score_thresh,
                         float nms_thresh, int max_det, const float reg_weights_host[4], int method, float sigma, float floor_thresh,
                         float *boxes_out, float *scores_out, int64_t *cls_out, int *src_out, int *num_out, void *workspace);

/* ============================== Panoptic tracking across frames ============================== */

/* One step of the tracker: associates the thing segments of frame `frame` (pan_2ch uint8 [H,W,3], channel 0 category with 255 =
 * VOID, channel 1 instance; a thing segment is (c, i) with c != 255, i >= 1) with the tracks the per-pixel memory remembers. The
 * reference has no tracking; the rule is this project's own (csrc/pan_track.hip, restated in tests/pan_track_ref.py):
 *   counts A_cur[c,i], A_mem[c,j], I[c,i,j] (same category only); candidates I > 0 and (double)I >= iou_thresh * (double)(A_cur +
 *   A_mem - I); per category greedy by IoU descending (I1 U2 against I2 U1 in int64, ties by ascending (i, j)); unmatched segments in
 *   ascending (c, i) take the first id of n_c mod 255 + 1, ... that is not live (in memory at the start of the step or assigned
 *   earlier in it) and leave n_c just past it, or -- all 255 live -- take over the unassigned memory track with the oldest frame index
 *   (smallest id on ties; n_c stays); out_2ch: thing pixels (c, id, 0), all others copied; memory: a pixel under a thing takes
 *   (track, frame); any other entry is cleared when its track was assigned in this step or frame - s > max_age.
 * memory: uint16 [H*W], c << 8 | j, 0 = none; zeroed by the caller before the first step. workspace:
 * upsnet_pan_track_workspace_bytes(H, W) bytes, ZEROED ONCE; every step leaves its count cells zero. The ints from
 * upsnet_pan_track_stamp_offset() bytes on are the tracker's state (stamp[65536]: frame index + 1 of a track's last assignment --
 * all memory pixels of a track share it --, cursor[256], scratch): zeroing them and `memory` resets the tracker.
 * The step's table has upsnet_pan_track_table_ints(H, W) ints: [0] = number of rows, [1] = frame, rows of 8 ints from [8] on, one per
 * current thing segment in ascending (c, i): c, i, id, matched, I, U, area, taken over (unmatched: I = 0, U = area). Frame t fills
 * the table at byte upsnet_pan_track_table_offset() + (t & 1) * 4 * table_ints of the workspace, so it outlives the next step.
 * host_table (may be NULL): pinned host memory; the head and the first min(host_rows, rows) rows are copied into it asynchronously
 * on `stream`. Three launches and the copy; nothing is synchronised or allocated.
 * Refused before any launch: a null pointer, H * W outside 1..2^24, iou_thresh outside [1/16, 1] (memory tracks are disjoint, so a
 * segment has at most 1 / iou_thresh <= 16 candidates, which bounds the LDS candidate list at 4080 per category), max_age < 0. */
size_t upsnet_pan_track_workspace_bytes(int height, int width);
size_t upsnet_pan_track_stamp_offset(void);
size_t upsnet_pan_track_table_ints(int height, int width);
size_t upsnet_pan_track_table_offset(void);
int upsnet_pan_track_step(void *stream, const unsigned char *pan_2ch, int height, int width, double iou_thresh, int max_age, int frame,
                          void *workspace, unsigned short *memory, unsigned char *out_2ch, int *host_table, int host_rows);

/* The same step with constant-velocity motion prediction (restated in tests/pan_track_motion_ref.py). For objects that
 * keep their motion from frame to frame; on erratic motion it matches fewer segments than the plain step. Integers throughout.
 * Every track (c, j) also keeps a centroid (cx, cy) = (floor(sum x / area), floor(sum y / area)) over the pixels it was last assigned
 * and a velocity (vx, vy) in pixels per frame. Step t:
 *   1. predict: a memory pixel (x, y) of track k, last assigned at frame s, votes for (x + vx (t - s), y + vy (t - s)), the shift in
 *      int64; a vote outside the image is dropped; among the votes on a pixel the smallest age t - s wins (ages compete as min(age,
 *      65535)), then the smallest key. The result, the predicted memory, holds at most one key per pixel, so the tracks stay disjoint
 *      and the candidate bound and iou_thresh >= 1/16 stand as they are.
 *   2. counts, candidates and the greedy matching of upsnet_pan_track_step, with A_mem and I counted on the predicted memory.
 *   3. "live" for the issue of new ids and the pool of tracks that may be taken over are those of the REAL memory: a track predicted
 *      off the image, or outvoted on all its pixels, has A_mem = 0 but is still remembered, and its id is not issued again.
 *   4. output map and memory update of upsnet_pan_track_step, on the real memory: it stays "the last seen mask, in place".
 *   5. every segment assigned in this step gives its track a new centroid; matched to a track last assigned at frame s, v = (c_new -
 *      c_old) / (t - s) per axis, truncated toward zero; newly issued or taken over, v = (0, 0). Any other track keeps both.
 * With all velocities zero the predicted memory is the real one and the step equals upsnet_pan_track_step bit for bit.
 * motion_workspace: upsnet_pan_track_motion_workspace_bytes(H, W) bytes, 16-byte aligned, ZEROED ONCE (zeroing it again, with the
 * tracker's state, resets the tracker): int32 (cx, cy, vx, vy) per key c << 8 | j from byte 0; the cells from byte
 * upsnet_pan_track_motion_count_offset() to upsnet_pan_track_motion_pred_offset() are zero after every step; from the latter on, one
 * uint32 per pixel, the predicted memory of the last step: 0 = none, else the key is 65535 - (value & 65535).
 * Seven launches (clear, predict, count, match, relabel, moments, velocities) and the copy; nothing is synchronised or allocated.
 * Refused before any launch: what upsnet_pan_track_step refuses, and a null or not 16-byte aligned motion_workspace. */
size_t upsnet_pan_track_motion_workspace_bytes(int height, int width);
size_t upsnet_pan_track_motion_count_offset(void);
size_t upsnet_pan_track_motion_pred_offset(void);
int upsnet_pan_track_step_motion(void *stream, const unsigned char *pan_2ch, int height, int width, double iou_thresh, int max_age, int frame,
                                 void *workspace, unsigned short *memory, unsigned char *out_2ch, int *host_table, int host_rows,
                                 void *motion_workspace);

/* Frame-stable colours of a 2-channel map, a pure function of (category, instance). mode 0: (R, G, B) = (category, instance, 1), VOID
 * (0,0,0). mode 1: stuff takes its category colour, a thing the offset rule of upsnet_pan_format with ordinal := instance and the
 * first attempt whose colour is not (0,0,0), no taken set. cat_table as in upsnet_pan_format (may be NULL in mode 0); an unknown
 * category is painted (0,0,0) in mode 1. One launch. */
int upsnet_pan_stable_colors(void *stream, const unsigned char *pred_2ch, int height, int width, const int *cat_table, int mode,
                             unsigned char *rgb);

/* ============================== Connected components of a panoptic map ============================== */

/* Labels the connected components of a 2-channel map (pan_2ch uint8 [H,W,3], channel 0 category with 255 = VOID, channel 1 instance)
 * and turns small fragments into VOID. The reference has no such step; the rule is this project's own (csrc/pan_components.hip,
 * restated in tests/pan_components_ref.py):
 *   - a pixel's key is c << 8 | i (bytes 0 and 1); byte 2 is never read and always preserved;
 *   - a pixel with c == 255 belongs to no component and is never changed;
 *   - a component is a maximal set of pixels of equal key connected under `connectivity` (4: edge neighbours, 8: corners too);
 *   - its label is the smallest linear index y * W + x among its pixels (VOID: -1), its area its pixel count;
 *   - the main component of a key is the one of largest area, ties to the smaller label;
 *   - a component is removed iff area < min_area and, with keep_largest != 0, it is not the main component of its key (so with
 *     keep_largest a key never vanishes entirely; without it small segments go too); min_area == 0 removes nothing;
 *   - every pixel of a removed component becomes (255, 0, byte 2), the VOID of upsnet_unified_pan_result; every other pixel keeps its
 *     bytes.
 * out_2ch may be pan_2ch itself. labels (may be NULL): int32 [H,W], 16-byte aligned, the labels of the INPUT map (a removed component
 * keeps its label there). stats: int32 [4] = distinct keys, components, components removed, pixels removed (all of the input map).
 * workspace: upsnet_pan_components_workspace_bytes(H, W) bytes, 16-byte aligned; its contents on entry are ARBITRARY and nothing
 * depends on an earlier call. Five launches, nothing is synchronised or allocated. Refused before any launch: a null pointer, H * W
 * outside 1..2^24 (the workspace size is then 0), connectivity other than 4 or 8, min_area < 0, a misaligned buffer. */
size_t upsnet_pan_components_workspace_bytes(int height, int width);
int upsnet_pan_components(void *stream, const unsigned char *pan_2ch, int height, int width, int connectivity, int min_area,
                          int keep_largest, void *workspace, unsigned char *out_2ch, int *labels, int *stats);

/* The absorbing mode of the same cleaning: a removed component takes the (category, instance) of the kept segment
 * it shares the longest border with and becomes VOID only where it has no such border. The rule is this project's own
 * (csrc/pan_components.hip, restated twice in tests/pan_absorb_ref.py):
 *   - keys, VOID, components, labels, areas, main components and which components are removed: exactly as upsnet_pan_components on
 *     the same arguments. A removed component is a FRAGMENT; every other component is KEPT;
 *   - votes: for every pixel p of a fragment r and every one of the four EDGE neighbours q of p inside the image (edge neighbours
 *     whatever `connectivity` is: border length is an edge notion): if q is not VOID and belongs to a kept component, the key of q
 *     gets one vote from r. One vote per pixel edge. VOID pixels, pixels outside the image and pixels of other fragments give none;
 *   - the donor of r is the key with the most votes, ties to the smaller key; no votes, no donor;
 *   - a fragment pixel with a donor becomes (donor category, donor instance, byte 2); one without becomes (255, 0, byte 2); every
 *     other pixel keeps its bytes;
 *   - a single round: a fragment that touches only other fragments, VOID or the image border, or kept pixels only across a corner,
 *     becomes VOID. Nothing is iterated.
 * Consequences: min_area == 0 is the identity; the result is a fixed point (an absorbed fragment is edge-adjacent to a kept pixel of
 * its new key and joins that kept component, so a second application removes nothing); the result differs from
 * upsnet_pan_components' exactly on the absorbed pixels.
 * out_2ch may be pan_2ch itself; labels (may be NULL) are those of the INPUT map. stats: int32 [8] = [0..3] as upsnet_pan_components
 * (distinct keys, components, fragments, fragment pixels), [4] fragments absorbed, [5] pixels absorbed, [6] distinct (fragment, donor
 * key) pairs that received a vote, [7] vote table overflow (0 or 1).
 * workspace: upsnet_pan_absorb_workspace_bytes(H, W) bytes, 16-byte aligned: that of upsnet_pan_components, one 64-bit winner cell per
 * pixel index, and the vote table of 2 H W slots (a 64-bit key and a 32-bit count each). A (fragment, key) pair needs a grid edge
 * between a fragment pixel and a kept pixel, and a map has 2HW - H - W edges: there are always fewer pairs than slots, so an insertion
 * cannot fail and stats[7] is 0. Should it ever be 1, out_2ch is a copy of pan_2ch and stats[2..5] are 0: the map is never silently
 * wrong. The workspace's contents on entry are ARBITRARY and nothing depends on an earlier call. Eight launches, nothing is
 * synchronised or allocated. Refused before any launch, as upsnet_pan_components refuses it: a null pointer, H * W outside 1..2^24 (the
 * workspace size is then 0), connectivity other than 4 or 8, min_area < 0, a misaligned buffer. */
size_t upsnet_pan_absorb_workspace_bytes(int height, int width);
int upsnet_pan_absorb(void *stream, const unsigned char *pan_2ch, int height, int width, int connectivity, int min_area, int keep_largest,
                      void *workspace, unsigned char *out_2ch, int *labels, int *stats);

/* ============================== Panoptic confidence: segment scores and the score filter ============================== */

/* Scores of the segments of a 2-channel map from a confidence plane (csrc/pan_confidence.hip; restated in
 * tests/pan_confidence_ref.py). pan_2ch uint8 [H,W,3] (key = byte 0 << 8 | byte 1; byte 0 == 255 is VOID, which is no segment and has
 * no row), conf uint8 [H,W] (upsnet_panoptic_fuse_up_conf's bytes, restored to the map's size). Per key: area = its pixels, sum_q = the
 * sum of their confidence bytes, both uint32 (H * W <= 2^24, so 255 * 2^24 < 2^32); the score of a segment is sum_q / (255 area),
 * which the host forms in double.
 *   table uint32 [upsnet_pan_segment_scores_table_ints()] (out): [0] = number of rows n, [1..3] = 0, then n rows (key, area, sum_q) in
 *   ascending key; rows past n are not written.
 * workspace: upsnet_pan_segment_scores_workspace_bytes() bytes, 4-byte aligned; its contents on entry are ARBITRARY. Three launches
 * (clear, count, compact), integer atomics only, nothing is synchronised or allocated. Refused before any launch: a null pointer, H * W
 * outside 1..2^24, a misaligned workspace or table. */
size_t upsnet_pan_segment_scores_workspace_bytes(void);
size_t upsnet_pan_segment_scores_table_ints(void);
int upsnet_pan_segment_scores(void *stream, const unsigned char *pan_2ch, const unsigned char *conf, int height, int width,
                              void *workspace, unsigned *table);

/* The score filter: every pixel of a non-VOID key whose row of `table` (upsnet_pan_segment_scores of the same map) has
 * (double)sum_q < min_score * (double)(255 * area) becomes (255, 0, 0); every other pixel keeps its three bytes (so does a key without a
 * row). One IEEE double product and no addition: numpy decides the same. 0 <= min_score <= 1 (0 removes nothing). out_2ch may be
 * pan_2ch itself. One launch, nothing is synchronised or allocated. */
int upsnet_pan_score_filter(void *stream, const unsigned char *pan_2ch, int height, int width, const unsigned *table, double min_score,
                            unsigned char *out_2ch);

/* ============================== Video metrics of tracked sequences: VPQ and STQ ============================== */

/* Video Panoptic Quality (Kim et al., Video Panoptic Segmentation, CVPR 2020) and Segmentation and Tracking Quality (Weber et al.,
 * STEP, NeurIPS 2021 datasets track). The reference has no video metric: the rules are this project's restatement of the published
 * definitions (csrc/video_eval.hip; restated in plain numpy in tests/video_pq_ref.py), never compared with a build of either tool.
 *
 * Per sequence. Prediction: one tracked 2-channel map per frame (uint8 [H,W,3], channel 0 category with 255 = VOID, channel 1
 * instance); a predicted TUBE is a key c << 8 | j with c != 255 (stuff: j = 0). Ground truth: one panoptic RGB map per frame (id = R +
 * 256 G + 65536 B, 0 = VOID) whose ids mean the same object in every frame, and the SEQUENCE TABLE: the union of the frames' segments
 * in ascending id, at most max_gt rows (id, category, iscrowd). Areas are always pixel counts. A GT pixel whose id is 0 or not in the
 * table is IGNORED.
 *
 * VPQ. For every window length n of `windows` (ascending, unique, each in 1..8) and every start s in 0..frames - n, summed over the n
 * frames: area_p[key], area_g[row], void[key] (pixels of the key on ignored GT), inter[row][key] counted only where cat(row) ==
 * cat(key). Then as _pq_compute_single_core treats one image:
 *   TP  non-crowd rows in ascending id, every key with inter > 0: iou = (double)inter / (double)(area_p + area_g - inter - void);
 *       iou > 0.5: tp[c]++, iou_sum[c] += iou, both matched;
 *   FN  every unmatched non-crowd row with area_g > 0 in the window: fn[c]++;
 *   FP  every unmatched key with area_p > 0 in the window: ign = void[key] + the sum of inter over ALL crowd rows of the key's
 *       category (a stated choice; upsnet_pq_accumulate keeps the reference's last-crowd-row rule); skipped iff (double)ign /
 *       (double)area_p > 0.5, else fp[c]++.
 * iou_sum accumulates in float64 in a fixed order: sequences in the order added, windows by ascending start, rows by ascending id.
 * tp / fp / fn / iou are [num_windows][256]; PQ per window length and the mean over `windows` are the host's (dataset/video_pq.py).
 *
 * STQ. Per sequence, over non-ignored pixels only, GT row r of category c_g, pred key (c_p, j):
 *   semantic     conf[c_g][c_p]++, pred VOID in column 255, crowd rows with their category, accumulated over all sequences; IoU_c =
 *                conf[c][c] / (row sum + column sum - conf[c][c]) for the categories whose denominator is > 0, iou their mean;
 *   association  GT tracks: thing, non-crowd rows; pred tracks: keys of a thing category; G[r] pixels of the GT track, P[key] pixels
 *                of the pred track on neither ignored nor thing-crowd GT, I[r][key] their joint pixels WHATEVER the categories;
 *                aq_sum = sum over r in ascending id of (1.0 / G[r]) * (sum over keys with I > 0 in ascending key of I * ((double)I /
 *                (double)(G + P - I))), float64; AQ = sum of aq_sum / max(number of GT tracks with G > 0, 1); STQ = sqrt(AQ * iou).
 * The device delivers the sequence's integer cells; the float64 operations of STQ run on the host from them.
 *
 * upsnet_video_eval_frame queues one frame: ONE pass over the pixels whatever `windows` is, the compaction of the frame's cells into
 * a ring of the last max_window frames and into the sequence-level table, and the window pass of every window that ends at this
 * frame -- three launches, no host read. table: device int [2 * num_rows + num_crowd]: per row in ascending id (id, category | iscrowd
 * << 8), then the indices of the crowd rows. windows: HOST ints. frame counts from 0 within the sequence; `sequence` and `frame` only
 * name the place in an error. cat_known uint8 [256]. status [2]: [0] bits 1 / 2 / 4: the frame table, the sequence table was full, a
 * window held more than 8192 list entries -- counts were dropped and the result is void (the caller raises); [1] starts as INT64_MAX
 * and takes the minimum of sequence << 32 | frame << 8 | category over pred categories that are not known.
 * upsnet_video_eval_end delivers the sequence: sequence_out (device, upsnet_video_eval_sequence_ints() ints): [0] = number of cells,
 * then from [2] on pairs (cell + 1, count), in arbitrary order; cell = kind << 28 | index with kind 0 JOINT (row << 16 | key), 1 AREA_P
 * (key), 2 VOID (key), 3 AREA_G (row), JOINT cells of every category pair. [1] and the ints past the last pair are unspecified
 * (the caller reads 2 + 2 * [0] ints). host_out (pinned, may be NULL) takes a copy, asynchronously.
 * workspace: upsnet_video_eval_workspace_bytes(max_gt, H, W, max_window) bytes (0: arguments out of range), ZEROED ONCE; the frame
 * tables are zero after every frame and all of it is zero after upsnet_video_eval_end. The frame table is sized from H * W (one slot
 * per 16 pixels, at least 4096); a sequence holds at most 32768 distinct cells and frames * H * W < 2^31 pixels.
 * Refused before any launch: a null pointer, H * W outside 1..2^24, max_gt outside 0..4096, more rows than max_gt, windows that are
 * not ascending, unique and in 1..max_window <= 8. */
size_t upsnet_video_eval_workspace_bytes(int max_gt, int height, int width, int max_window);
size_t upsnet_video_eval_sequence_ints(void);
int upsnet_video_eval_frame(void *stream, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                            const int *table, int num_rows, int num_crowd, int max_gt, const int *windows, int num_windows, int max_window,
                            int frame, int sequence, const unsigned char *cat_known, void *workspace, int64_t *tp, int64_t *fp, int64_t *fn,
                            double *iou, uint64_t *status);
int upsnet_video_eval_end(void *stream, int height, int width, int max_gt, int max_window, void *workspace, int *sequence_out,
                          int *host_out);

/* ============================== MOTS measures of tracked sequences ============================== */

/* sMOTSA, MOTSA, MOTSP, IDS, Frag and MT / PT / ML (Voigtlaender et al., MOTS: Multi-Object Tracking and Segmentation, CVPR 2019).
 * The reference has no video metric: the rules are this project's restatement of the published definitions (csrc/mots_eval.hip;
 * restated in plain numpy in tests/mots_ref.py), never compared with a build of mots_tools.
 *
 * Per sequence. Prediction, ground truth and the SEQUENCE TABLE are exactly those of upsnet_video_eval_frame: a tracked 2-channel map
 * and a panoptic RGB map (id = R + 256 G + 65536 B) per frame, the table the union of the frames' segments in ascending id. The scored
 * categories are the THING categories. For a thing category c at frame t:
 *   GT objects   the non-crowd rows of category c; a row is PRESENT at t iff it has at least one pixel in frame t;
 *   ignore(c)    the GT pixels whose id is 0 or not in the table, plus the pixels of every crowd row of category c (crowd rows of
 *                other categories and stuff rows are not ignore);
 *   hypotheses   the keys c << 8 | j with at least one pixel in frame t, whatever j;
 *   match        row r and key k of the same category match iff 3 * I > A_g + A_p in int64: IoU > 0.5 on the whole masks (ignore pixels
 *                are not taken out of the union). Each row and each key has at most one partner: I <= A_p gives 2 * I > A_g, and two
 *                disjoint keys cannot each cover more than half of one row (and the same with the sides exchanged);
 *   counts       per match tp[c]++ and soft[c] += (double)I / (double)(A_g + A_p - I); per present, unmatched row fn[c]++; per present
 *                row gt_masks[c]++; per unmatched key fp[c]++, unless 2 * ign > A_p, ign the key's pixels on ignore(c): then
 *                fp_ignored[c]++ instead;
 *   identity     per row, `last` is the key it last matched, in any earlier frame, across gaps and absences; a match with `last` set
 *                and different from k: ids[c]++; then last = k;
 *   fragments    per row, `gap` is set when the row is present and unmatched after it has been matched at least once; a match with
 *                `gap` set: frag[c]++, and gap is cleared;
 *   coverage     present[r] and tracked[r] count frames; at the end of the sequence every row with present > 0 is MT iff 5 * tracked
 *                > 4 * present, ML iff 5 * tracked < present, else PT.
 * soft accumulates in float64 in a fixed order: sequences in the order added, frames in order, rows by ascending id. MOTSA = (tp - fp -
 * ids) / max(gt_masks, 1), sMOTSA = (soft - fp - ids) / max(gt_masks, 1), MOTSP = soft / max(tp, 1) are the host's (dataset/mots.py).
 *
 * upsnet_mots_eval_frame queues one frame: one pass over the pixels, the match pass over the frame's cells and the row-state pass --
 * three launches, no host read. table: device int [2 * num_rows]: per row in ascending id (id, category | iscrowd << 8 | isthing << 9).
 * cat_info uint8 [256]: bit 0 the category is known, bit 1 it is a thing. counts: int64 [7][256] = tp, fp, fn, gt_masks, ids, frag,
 * fp_ignored; soft: double [256]. frame counts from 0 within the sequence and also selects one of two list headers by its parity, so
 * frames must be queued in order; `sequence` only names the place in an error. status [2]: [0] bit 1: the frame table was full -- counts
 * were dropped and the result is void (the caller raises); [1] starts as INT64_MAX and takes the minimum of sequence << 32 | frame << 8
 * | category over pred categories that are not known.
 * upsnet_mots_eval_end ends the sequence: mtl int64 [3][256] takes MT, PT, ML per category (added); one launch.
 * workspace: upsnet_mots_eval_workspace_bytes(max_gt, H, W) bytes (0: arguments out of range), ZEROED ONCE; everything but the four
 * state words per row is zero after every frame and all of it is zero after upsnet_mots_eval_end. The frame table is sized from H * W
 * (one slot per 16 pixels, at least 4096).
 * Refused before any launch: a null pointer, H * W outside 1..2^24, max_gt outside 0..4096, more rows than max_gt, frame outside
 * 0..2^24-1, sequence outside 0..2^30-1, a workspace that is not 8-byte aligned. */
size_t upsnet_mots_eval_workspace_bytes(int max_gt, int height, int width);
int upsnet_mots_eval_frame(void *stream, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                           const int *table, int num_rows, int max_gt, int frame, int sequence, const unsigned char *cat_info,
                           void *workspace, int64_t *counts, double *soft, uint64_t *status);
int upsnet_mots_eval_end(void *stream, int height, int width, const int *table, int num_rows, int max_gt, void *workspace, int64_t *mtl);

/* COCO RLE of every thing segment of one 2-channel map (a key c << 8 | i with c != 255 and i >= 1, as in upsnet_pan_track_step): the
 * positions p = x * height + y of the column-major flattening at which the membership of the key changes, the wrap from one column's
 * last pixel to the next column's first counting as adjacent; a segment that holds pixel 0 has a change at 0, none is reported at
 * height * width. pairs[i] = key << 24 | p for i < min(*count, cap), in arbitrary order (sorting them gives every segment's positions in
 * ascending order, segments by ascending key); *count is the number of changes even when it exceeds cap, so the caller grows pairs and
 * calls again. One memset and one launch. Refused before any launch: a null pointer, height * width outside 1..2^24, cap < 0. */
int upsnet_pan_rle_transitions(void *stream, const unsigned char *pan_2ch, int height, int width, int cap, int64_t *pairs, int *count);

#ifdef __cplusplus
}
#endif
#endif /* UPSNET_HIP_H */
