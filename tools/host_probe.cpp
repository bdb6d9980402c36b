// host_probe.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_host_probe_cpu.py): the HOST half of libupsnet_hip under ASan + UBSan.
//
// Links the host-instrumented twin of the library (python -m upsnet_amd.build --host-sanitize) and calls only what returns before
// any device call, so it needs no GPU and opens none:
//   Q lines  every size / capacity / geometry query of include/upsnet_hip.h over a grid of its integer arguments -- 0, 1, the
//            documented maximum, one above it, INT_MAX, and pairs whose product passes 2^31 and 2^32:
//                Q <name> <sweep> <mono> <a0,a1,...> -> <value>
//            <sweep>: s<k> = argument k grows, the others stay at the base row; j = a joint row. <mono>: 1 where growing that
//            argument may never shrink the answer (sizes and counts), 0 where it may (strides, kernel sizes, flags).
//   R lines  every launching entry point with arguments its own checks must refuse -- all pointers null first, then dummy non-null
//            pointers with one out-of-contract dimension:
//                R <name> <tag> ret=<r> hip=<0|1> msg=<upsnet_last_error()>
//            hip=1: the message carries a HIP runtime error string, i.e. the call got as far as the runtime instead of refusing.
// A sanitizer report ends the program with a non-zero status (-fno-sanitize-recover=all).
#include <climits>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

extern "C" {
#include "upsnet_hip.h"
}

typedef std::vector<long> V;

// ------------------------------------------------------------------------------------------------------------------ queries
template <class R, class... A, size_t... I>
static long long call_with(R (*f)(A...), const V &v, std::index_sequence<I...>) { return (long long)f((A)v[I]...); }

static void print_q(const char *name, const char *sweep, int mono, const V &v, long long value)
{
    std::printf("Q %s %s %d ", name, sweep, mono);
    for (size_t i = 0; i < v.size(); ++i) std::printf("%s%ld", i ? "," : "", v[i]);
    std::printf(" -> %lld\n", value);
}

struct Sweep { int arg, mono; V vals; };

template <class R, class... A>
static void query(const char *name, R (*f)(A...), const V &base, const std::vector<Sweep> &sweeps, const std::vector<V> &joint = {})
{
    if (base.size() != sizeof...(A)) { std::printf("BAD %s: %zu base values for %zu arguments\n", name, base.size(), sizeof...(A)); return; }
    for (size_t k = 0; k < sweeps.size(); ++k) {
        char tag[16];
        std::snprintf(tag, sizeof tag, "s%zu", k);
        for (long x : sweeps[k].vals) {
            V v = base;
            v[sweeps[k].arg] = x;
            print_q(name, tag, sweeps[k].mono, v, call_with(f, v, std::index_sequence_for<A...>{}));
        }
    }
    for (const V &v : joint) print_q(name, "j", 0, v, call_with(f, v, std::index_sequence_for<A...>{}));
}

template <class R> static void query0(const char *name, R (*f)(void)) { print_q(name, "j", 0, V{}, (long long)f()); }

static const long IMAX = INT_MAX;
static const V DIM = {0, 1, 2, 64, 1000, 4096, 4097, 32768, 32769, 46341, 65536, 1L << 24, IMAX};     // a height or a width
static const V CNT = {0, 1, 2, 100, 256, 257, 1000, 2048, 4096, 4097, 8192, 8193, 65535, 65536, 65537, 1L << 24, IMAX};   // a count
static const V CH = {0, 1, 32, 256, 2048, 65536, IMAX};                                               // a channel count
static const V KS = {0, 1, 2, 3, 5, 7};                                                               // kernel side, stride, dilation, pad
static const V LNG = {0, 1, 1000, 1L << 24, (1L << 24) + 1, 1L << 31, 1L << 32, 1L << 40};             // a long total
static const V FLAG = {0, 1};
// (height, width) pairs whose product passes 2^24, 2^30, 2^31 and 2^32
static const std::vector<std::pair<long, long>> HW = {{4096, 4096}, {4096, 4097}, {32768, 32768}, {46340, 46341}, {46341, 46341},
                                                       {65536, 65536}, {IMAX, 2}, {IMAX, IMAX}};

static std::vector<V> hw_rows(V base, int ih, int iw)
{
    std::vector<V> r;
    for (auto &p : HW) { V v = base; v[ih] = p.first; v[iw] = p.second; r.push_back(v); }
    return r;
}

static void queries()
{
#define Q(name, ...) query(#name, upsnet_##name, __VA_ARGS__)
    Q(dcn_packed_weight_floats, V{256, 256, 3, 3}, {{0, 1, CH}, {1, 1, CH}, {2, 1, KS}, {3, 1, KS}}, {V{IMAX, IMAX, 7, 7}, V{-1, 256, 3, 3}});
    Q(dcn_packed_weight_bf16_elems, V{256, 256, 3, 3}, {{0, 1, CH}, {1, 1, CH}, {2, 1, KS}, {3, 1, KS}}, {V{IMAX, IMAX, 7, 7}, V{-1, 256, 3, 3}});
    Q(deform_conv_fused_splitk_workspace_bytes, V{64, 96, 256, 3, 3, 1, 1, 1, 4},
      {{0, 1, DIM}, {1, 1, DIM}, {2, 1, CH}, {3, 0, KS}, {4, 0, KS}, {5, 1, KS}, {6, 0, V{0, 1, 2, 3, IMAX}}, {7, 0, KS}, {8, 1, V{0, 1, 2, 16, 65536, IMAX}}},
      hw_rows(V{0, 0, 256, 3, 3, 1, 1, 1, 4}, 0, 1));
    Q(conv2d_splitk_workspace_bytes, V{2, 64, 96, 256, 3, 3, 1, 1, 4},
      {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}, {3, 1, CH}, {4, 0, KS}, {5, 0, KS}, {6, 0, V{0, 1, 2, 3, IMAX}}, {7, 1, KS}, {8, 1, V{0, 1, 2, 16, 65536, IMAX}}},
      hw_rows(V{2, 0, 0, 256, 3, 3, 1, 1, 4}, 1, 2));
    Q(conv2d_winograd36_splitk_workspace_bytes, V{2, 64, 96, 256, 4}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}, {3, 1, CH}, {4, 1, V{0, 1, 2, 16, 65536, IMAX}}},
      hw_rows(V{2, 0, 0, 256, 4}, 1, 2));
    Q(conv1x1_splitk_workspace_bytes, V{2, 64, 96, 256, 4}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}, {3, 1, CH}, {4, 1, V{0, 1, 2, 16, 65536, IMAX}}},
      hw_rows(V{2, 0, 0, 256, 4}, 1, 2));
    Q(conv1x1_ksw_packed_weight_floats, V{256, 256}, {{0, 1, CH}, {1, 1, CH}}, {V{IMAX, IMAX}, V{-1, 1}});
    Q(conv3x3_ksw_packed_weight_floats, V{256}, {{0, 1, CH}}, {V{-1}});
    Q(nms_workspace_bytes, V{5, 1000}, {{0, 1, CNT}, {1, 1, CNT}}, {V{32768, 65536}, V{46341, 46341}, V{65536, 65536}, V{IMAX, IMAX}, V{-1, 5}});
    Q(soft_nms_batched_workspace_bytes, V{5, 8192}, {{0, 1, CNT}, {1, 1, CNT}}, {V{32768, 65536}, V{46341, 46341}, V{65536, 65536}, V{IMAX, IMAX}});
    Q(soft_nms_workspace_bytes, V{1000}, {{0, 1, CNT}});
    Q(mask_roi_capacity, V{1000, 9, 0}, {{0, 1, CNT}, {1, 1, V{0, 1, 2, 9, 81, 82, 65536, IMAX}}, {2, 0, FLAG}}, {V{1000, 9, 1}, V{IMAX, IMAX, 0}, V{IMAX, IMAX, 1}, V{46341, 46342, 0}});
    Q(mask_roi_workspace_bytes, V{1000, 9, 0}, {{0, 1, CNT}, {1, 1, V{0, 1, 2, 9, 81, 82, 65536, IMAX}}, {2, 0, FLAG}}, {V{1000, 9, 1}, V{IMAX, IMAX, 0}, V{IMAX, IMAX, 1}, V{46341, 46342, 0}});
    Q(mask_roi_soft_workspace_bytes, V{1000, 9}, {{0, 1, CNT}, {1, 1, V{0, 1, 2, 9, 81, 82, 65536, IMAX}}}, {V{IMAX, IMAX}, V{8192, 65536}});
    Q(mask_removal_workspace_bytes, V{100, 8, 64, 96}, {{0, 1, CNT}, {1, 1, V{0, 1, 8, 80, 65536, IMAX}}, {2, 1, DIM}, {3, 1, DIM}}, hw_rows(V{100, 8, 0, 0}, 2, 3));
    query0("unified_pan_workspace_bytes", upsnet_unified_pan_workspace_bytes);
    Q(combined_pan_workspace_bytes, V{4, 1 << 20}, {{0, 1, CNT}, {1, 1, LNG}}, {V{IMAX, 1L << 40}, V{-1, 5}, V{4, -1}});
    Q(pq_workspace_bytes, V{100}, {{0, 1, CNT}}, {V{-1}});
    Q(pan_boundary_workspace_bytes, V{64, 96}, {{0, 1, DIM}, {1, 1, DIM}}, hw_rows(V{0, 0}, 0, 1));
    Q(pq_boundary_workspace_bytes, V{100, 64, 96}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}}, hw_rows(V{100, 0, 0}, 1, 2));
    Q(det_eval_image_workspace_bytes, V{100, 100, 50, 64, 96, 1}, {{0, 1, CNT}, {1, 1, CNT}, {2, 1, CNT}, {3, 1, DIM}, {4, 1, DIM}, {5, 0, FLAG}},
      hw_rows(V{100, 100, 50, 0, 0, 1}, 3, 4));
    Q(det_eval_boundary_image_workspace_bytes, V{100, 100, 50, 64, 96}, {{0, 1, CNT}, {1, 1, CNT}, {2, 1, CNT}, {3, 1, DIM}, {4, 1, DIM}},
      hw_rows(V{100, 100, 50, 0, 0}, 3, 4));
    Q(det_eval_accumulate_workspace_bytes, V{1000, 100}, {{0, 1, LNG}, {1, 1, CNT}}, {V{1L << 40, IMAX}, V{-1, 100}, V{1000, 0}});
    Q(boundary_dilation_fits, V{64, 96, 2}, {{0, 0, DIM}, {1, 0, DIM}, {2, 0, CNT}}, hw_rows(V{0, 0, 2}, 0, 1));
    Q(boundary_masks_workspace_bytes, V{10, 64, 96}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}}, hw_rows(V{10, 0, 0}, 1, 2));
    Q(poly_raster_workspace_bytes, V{100, 1000}, {{0, 0, V{0, 1, 1000, 1001}}, {1, 1, V{100, 1000, 1L << 24, (1L << 24) + 1, 1L << 31, 1L << 32, 1L << 40}}},
      {V{1L << 24, 1L << 24}, V{-1, 5}, V{5, -1}});
    Q(proposal_recall_workspace_bytes, V{4, 1 << 20}, {{0, 1, CNT}, {1, 1, LNG}}, {V{IMAX, 1L << 40}, V{-1, 5}, V{4, -1}});
    Q(cs_inst_counts_ints, V{100}, {{0, 1, CNT}}, {V{-1}});
    Q(cs_inst_workspace_bytes, V{100}, {{0, 1, CNT}}, {V{-1}});
    query0("cs_inst_state_words", upsnet_cs_inst_state_words);
    query0("cs_pixel_inst_ints", upsnet_cs_pixel_inst_ints);
    query0("pan_format_workspace_bytes", upsnet_pan_format_workspace_bytes);
    query0("pan_format_table_ints", upsnet_pan_format_table_ints);
    Q(gt_prepare_workspace_bytes, V{100}, {{0, 1, CNT}}, {V{-1}});
    Q(vis_workspace_bytes, V{10, 64, 96}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}}, hw_rows(V{10, 0, 0}, 1, 2));
    query0("pan_vis_workspace_bytes", upsnet_pan_vis_workspace_bytes);
    query0("group_norm_chunk_pixels", upsnet_group_norm_chunk_pixels);
    Q(pan_track_workspace_bytes, V{64, 96}, {{0, 1, DIM}, {1, 1, DIM}}, hw_rows(V{0, 0}, 0, 1));
    Q(pan_track_table_ints, V{64, 96}, {{0, 1, DIM}, {1, 1, DIM}}, hw_rows(V{0, 0}, 0, 1));
    Q(pan_track_motion_workspace_bytes, V{64, 96}, {{0, 1, DIM}, {1, 1, DIM}}, hw_rows(V{0, 0}, 0, 1));
    Q(pan_components_workspace_bytes, V{64, 96}, {{0, 1, DIM}, {1, 1, DIM}}, hw_rows(V{0, 0}, 0, 1));
    Q(pan_absorb_workspace_bytes, V{64, 96}, {{0, 1, DIM}, {1, 1, DIM}}, hw_rows(V{0, 0}, 0, 1));
    query0("pan_segment_scores_workspace_bytes", upsnet_pan_segment_scores_workspace_bytes);
    query0("pan_segment_scores_table_ints", upsnet_pan_segment_scores_table_ints);
    Q(video_eval_workspace_bytes, V{100, 64, 96, 2}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}, {3, 1, V{0, 1, 2, 8, 9, IMAX}}}, hw_rows(V{100, 0, 0, 2}, 1, 2));
    query0("video_eval_sequence_ints", upsnet_video_eval_sequence_ints);
    Q(mots_eval_workspace_bytes, V{100, 64, 96}, {{0, 1, CNT}, {1, 1, DIM}, {2, 1, DIM}}, hw_rows(V{100, 0, 0}, 1, 2));
#undef Q
    // the two queries that take arrays: (levels | maps) x a size, every map of the same size
    for (long nlev : V{0, 1, 5, 8, 9})
        for (long side : V{0, 1, 64, 4096, 46341, 65536, IMAX})
            for (long pre : V{0, 1, 1000, 8192, 8193, IMAX}) {
                int h[16], w[16];
                for (int i = 0; i < 16; ++i) h[i] = w[i] = (int)side;
                if (pre != 1000 && side != 64) continue;
                print_q("proposal_workspace_bytes", "j", 0, V{nlev, side, side, 3, pre, 1000},
                        (long long)upsnet_proposal_workspace_bytes((int)nlev, h, w, 3, (int)pre, 1000));
            }
    print_q("proposal_workspace_bytes", "j", 0, V{5, -1, -1, 3, 1000, 1000}, (long long)upsnet_proposal_workspace_bytes(5, nullptr, nullptr, 3, 1000, 1000));
    for (long nseg : V{0, 1, 5, 6})
        for (long nb : V{0, 1, 2, 65536, IMAX})
            for (auto &p : std::vector<std::pair<long, long>>{{0, 0}, {1, 1}, {64, 96}, {46341, 46341}, {65536, 65536}, {IMAX, IMAX}, {-1, 4}}) {
                int b[8], h[8], w[8];
                for (int i = 0; i < 8; ++i) { b[i] = (int)nb; h[i] = (int)p.first; w[i] = (int)p.second; }
                print_q("group_norm_workspace_bytes", "j", 0, V{nseg, nb, p.first, p.second},
                        (long long)upsnet_group_norm_workspace_bytes((int)nseg, b, h, w));
            }
}

// ---------------------------------------------------------------------------------------------------------------- refusals
static std::vector<std::string> hip_errors;

static int report(const char *name, const char *tag, int ret, bool print = true)
{
    const char *msg = upsnet_last_error();
    int hip = 0;
    for (const std::string &e : hip_errors)
        if (std::strstr(msg, e.c_str())) hip = 1;
    if (print) std::printf("R %s %s ret=%d hip=%d msg=%s\n", name, tag, ret, hip, msg);
    return ret != 0 && hip;
}

// every argument value-initialised: null pointers, zero sizes
template <class... A> static void refuse_null(const char *name, int (*f)(A...)) { report(name, "null", f(A{}...)); }

// generated calls: every pointer argument = pv, every integer (and float) argument = iv, except the (position, value) pairs in ov
struct Ov { int arg; long val; };
template <class T> static T gen(long iv, void *pv)
{
    if constexpr (std::is_pointer_v<T>) return (T)pv;
    else return (T)iv;
}
template <class... A, size_t... I>
static int call_gen(int (*f)(A...), long iv, void *pv, const std::vector<Ov> &ov, std::index_sequence<I...>)
{
    long v[sizeof...(A) + 1];
    for (size_t i = 0; i < sizeof...(A); ++i) v[i] = iv;
    for (const Ov &o : ov) v[o.arg] = o.val;
    return f(gen<A>(v[I], pv)...);
}
// The pointer checks, by difference: find one size s such that the call with every size = s and every pointer NON-null passes all
// argument checks (it gets as far as the runtime, which has no device), then make the same call with every pointer null. A refusal
// of that second call can only be for the pointers. Tag null_ptr; where no uniform size is valid (null_ptr_msg) the call is made
// with sizes of 1 and the message itself has to speak of a null pointer.
template <class... A> static void refuse_null_ptr(const char *name, int (*f)(A...), void *pv, long iv = 0, const std::vector<Ov> &ov = {})
{
    if (iv) {    // sizes given by hand: the same difference
        const bool valid = report(name, "", call_gen(f, iv, pv, ov, std::index_sequence_for<A...>{}), false);
        report(name, valid ? "null_ptr" : "null_ptr_msg", call_gen(f, iv, nullptr, ov, std::index_sequence_for<A...>{}));
        return;
    }
    for (long s : {1L, 64L, 128L, 2L, 4L, 256L, 32L}) {
        if (!report(name, "", call_gen(f, s, pv, {}, std::index_sequence_for<A...>{}), false)) continue;
        report(name, "null_ptr", call_gen(f, s, nullptr, {}, std::index_sequence_for<A...>{}));
        return;
    }
    report(name, "null_ptr_msg", call_gen(f, 1, nullptr, {}, std::index_sequence_for<A...>{}));
}
template <class... A>
static void refuse_gen(const char *name, const char *tag, int (*f)(A...), long iv, void *pv, const std::vector<Ov> &ov = {})
{
    report(name, tag, call_gen(f, iv, pv, ov, std::index_sequence_for<A...>{}));
}

// The non-null pointer of every row: never written and never passed to a launch, since every row must be refused first. A launcher may
// read an array argument on the host (sizes, per-map pointers): every 32-bit word is 1, so it reads sizes of 1 and non-null pointers.
alignas(16) static int dummy_words[4096];
static float *const dummy = (float *)dummy_words;
static float *const D = dummy;
static const float *const DP[5] = {D, D, D, D, D};
static float *const DO[5] = {D, D, D, D, D};
static const void *const DVP[5] = {D, D, D, D, D};
static void *const DVO[5] = {D, D, D, D, D};

static void refusals()
{
    for (int e = 1; e < 2000; ++e) {
        const char *s = hipGetErrorString((hipError_t)e);
        if (s && *s && !std::strstr(s, "nrecognized") && !std::strstr(s, "nknown")) hip_errors.push_back(s);
    }
    for (int &w : dummy_words) w = 1;
    // per launcher: all-zero arguments; valid sizes with every pointer null (refuse_null_ptr); non-null pointers with every size -1
#define N(name) refuse_null("upsnet_" #name, upsnet_##name); refuse_null_ptr("upsnet_" #name, upsnet_##name, D); \
    refuse_gen("upsnet_" #name, "bad_dim", upsnet_##name, -1, D);
    N(zero_fill) N(roi_align_forward) N(roi_align_forward_nhwc) N(fpn_roi_align_forward) N(fpn_roi_order)
    N(fpn_roi_align_forward_ordered) N(deform_im2col) N(mod_deform_im2col) N(roi_align_backward) N(deform_col2im)
    N(deform_col2im_coord) N(mod_deform_col2im) N(mod_deform_col2im_coord) N(deform_conv_forward_nhwc) N(dcn_pack_weight)
    N(deform_conv_fused_nhwc) N(deform_conv_fused_nhwc_splitk) N(dcn_pack_weight_bf16) N(deform_conv_fused_nhwc_bf16)
    N(prep_image_u8) N(image_to_nhwc4) N(conv2d_nhwc_f32_multiw) N(conv2d_nhwc_f32) N(conv2d_nhwc_f32_splitk)
    N(conv2d_winograd_nhwc_f32) N(conv2d_winograd_nhwc_f32_splitk) N(conv_pack_weight_winograd) N(conv2d_winograd_nhwc_f32_tn32)
    N(conv_pack_weight_winograd_tn32) N(conv2d_winograd_nhwc_f32_tail) N(conv2d_nhwc_bf16) N(conv_pack_weight_bf16)
    N(bottleneck_proj_bf16) N(stem_pool_pack_weight_f32) N(stem_pool_f32) N(stem_pool_pack_weight_bf16) N(stem_pool_bf16)
    N(deconv2x2_nhwc_bf16) N(bottleneck_bf16) N(conv2d_stem_nhwc4_f32) N(conv_pack_weight_stem) N(deconv2x2_nhwc_f32)
    N(deconv2x2_pack_weight) N(deconv2x2_frag_nhwc_f32) N(conv_pack_weight) N(conv1x1_frag_nhwc_f32)
    N(conv1x1_siblings_nhwc_f32) N(conv2d_winograd36_nhwc_f32) N(conv_pack_weight_winograd36)
    N(conv2d_winograd36_nhwc_f32_splitk) N(conv1x1_ksw_pack_weight) N(conv1x1_ksw_nhwc_f32) N(conv3x3_ksw_pack_weight)
    N(conv3x3_ksw_nhwc_f32) N(conv1x1_frag_nhwc_f32_splitk) N(conv1x1_pair_nhwc_f32) N(nms_batched) N(cpu_nms_batched)
    N(soft_nms_batched) N(soft_nms) N(pyramid_proposals) N(pyramid_proposals_strided) N(pyramid_proposals_strided_ordered)
    N(pyramid_proposals_joint_strided) N(mask_roi) N(mask_roi_ex) N(mask_roi_dedup) N(mask_logit_gather) N(mask_removal)
    N(panoptic_tail_pack) N(mask_paste) N(seg_term) N(panoptic_fuse) N(fcn_score_combine) N(panoptic_fuse_up)
    N(panoptic_fuse_up_conf) N(panoptic_argmax) N(unified_pan_result) N(combined_pan_result) N(im_post_rle)
    N(restore_label_maps) N(restore_plane_u8) N(pq_accumulate) N(pan_boundary_map) N(pq_boundary_accumulate)
    N(confusion_accumulate) N(det_eval_image) N(det_eval_accumulate) N(det_eval_boundary_image) N(boundary_masks) N(poly_raster)
    N(proposal_recall) N(cs_inst_image) N(cs_pixel_image) N(pan_format) N(pan_relabel) N(gt_prepare) N(vis_render) N(pan_vis)
    N(group_norm_nhwc_f32) N(group_norm_small_nhwc_f32) N(cs_inst_expand) N(tta_seg_merge) N(tta_roi_union) N(tta_boxes_to_aug)
    N(tta_mask_merge) N(box_vote) N(mask_roi_soft) N(pan_track_step) N(pan_track_step_motion) N(pan_stable_colors)
    N(pan_components) N(pan_absorb) N(pan_segment_scores) N(pan_score_filter) N(video_eval_frame) N(video_eval_end)
    N(mots_eval_frame) N(mots_eval_end) N(pan_rle_transitions)
#undef N
    // launchers whose checks name sizes and pointers in one message and accept no uniform size: valid sizes by hand
#define P(name, iv, ...) refuse_null_ptr("upsnet_" #name, upsnet_##name, D, iv, __VA_ARGS__)
    P(conv_pack_weight_stem, 64, {{3, 3}, {4, 7}, {5, 7}});
    P(deconv2x2_pack_weight, 32, {{4, 128}});
    P(deconv2x2_nhwc_f32, 32, {{2, 1}, {7, 128}, {10, 0}});
    P(conv2d_winograd36_nhwc_f32, 64, {{1, 1}, {12, 0}});
    P(conv2d_winograd36_nhwc_f32_splitk, 64, {{3, 1}, {11, 0}, {12, 2}});
    P(conv1x1_ksw_nhwc_f32, 64, {{4, 1}, {11, 1}, {12, 0}, {13, 32}, {14, 32}, {15, 0}});
    P(conv2d_winograd_nhwc_f32_tail, 64, {{3, 2}, {4, 1}, {5, 8}, {6, 8}, {11, 32}, {13, 32}, {14, 0}});
#undef P
    refuse_null("upsnet_nms_host", upsnet_nms_host);
    refuse_gen("upsnet_nms_host", "null_ptr_msg", upsnet_nms_host, 1, nullptr);      // (host pointers: it would read the boxes)
    refuse_gen("upsnet_nms_host", "bad_dim", upsnet_nms_host, -1, D);
    // the two whose all-zero call is a documented no-op (nothing to fill, no problems): one size up, pointers still null
    report("upsnet_zero_fill", "null", upsnet_zero_fill(nullptr, nullptr, 16));
    report("upsnet_proposal_recall", "null", upsnet_proposal_recall(nullptr, 1, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr));

    // ---- the convolution family: (tag: what is out of contract)
    const int one[1] = {1}, h64[1] = {64}, w96[1] = {96}, h2[1] = {2}, n4096[1] = {4096}, h8192[1] = {8192}, w2048[1] = {2048}, w2047[1] = {2047},
              w4095[1] = {4095};
#define R(name, tag, ...) report("upsnet_" #name, tag, upsnet_##name(__VA_ARGS__))
    // conv2d_nhwc_f32(stream, nseg, x, residual, out, batch, height, width, Cin, wpack, ldw, bias, Cout, KH, KW, stride, pad, relu, residual_up)
    R(conv2d_nhwc_f32, "cin_not_32", nullptr, 1, DP, nullptr, DO, one, h64, w96, 48, D, 64, D, 64, 3, 3, 1, 1, 0, 0);
    R(conv2d_nhwc_f32, "ldw_below_cout", nullptr, 1, DP, nullptr, DO, one, h64, w96, 64, D, 32, D, 64, 3, 3, 1, 1, 0, 0);
    R(conv2d_nhwc_f32, "empty_output", nullptr, 1, DP, nullptr, DO, one, h2, h2, 64, D, 64, D, 64, 7, 7, 1, 0, 0, 0);
    R(conv2d_nhwc_f32, "input_2^30", nullptr, 1, DP, nullptr, DO, one, h8192, n4096, 32, D, 32, D, 32, 3, 3, 1, 1, 0, 0);              // exactly 2^30 floats
    R(conv2d_nhwc_f32, "output_2^29", nullptr, 1, DP, nullptr, DO, one, n4096, w2048, 32, D, 64, D, 64, 1, 1, 1, 0, 0, 0);         // exactly 2^29 floats out
    R(conv2d_nhwc_f32_multiw, "cin_not_32", nullptr, 1, DP, DO, one, h64, w96, 48, DP, 64, 64, 3, 3, 1, 1, 0);
    R(conv2d_nhwc_f32_multiw, "input_2^30", nullptr, 1, DP, DO, one, h8192, n4096, 32, DP, 32, 32, 3, 3, 1, 1, 0);
    R(conv2d_nhwc_f32_splitk, "cin_not_32", nullptr, D, nullptr, D, 1, 64, 96, 48, D, 64, D, 64, 3, 3, 1, 1, 0, 2, D);
    R(conv2d_nhwc_f32_splitk, "input_2^30", nullptr, D, nullptr, D, 1, 8192, 4096, 32, D, 32, D, 32, 3, 3, 1, 1, 0, 2, D);
    R(conv2d_winograd_nhwc_f32, "cin_not_32", nullptr, 1, DP, nullptr, DO, one, h64, w96, 48, D, 64, D, 64, 0);
    R(conv2d_winograd_nhwc_f32, "ldw_below_cout", nullptr, 1, DP, nullptr, DO, one, h64, w96, 64, D, 32, D, 64, 0);
    R(conv2d_winograd_nhwc_f32, "input_2^30", nullptr, 1, DP, nullptr, DO, one, h8192, n4096, 32, D, 32, D, 32, 0);
    R(conv2d_winograd_nhwc_f32, "output_2^29", nullptr, 1, DP, nullptr, DO, one, n4096, w2048, 32, D, 64, D, 64, 0);
    R(conv2d_winograd_nhwc_f32_tn32, "input_2^30", nullptr, 1, DP, nullptr, DO, one, h8192, n4096, 32, D, 32, D, 32, 0);
    R(conv2d_winograd_nhwc_f32_splitk, "input_2^30", nullptr, D, nullptr, D, 1, 8192, 4096, 32, D, 32, D, 32, 0, 2, D);
    R(conv2d_winograd36_nhwc_f32, "cin_not_32", nullptr, 1, DP, DO, one, h64, w96, 48, D, 64, D, 64, 0);
    R(conv2d_winograd36_nhwc_f32, "input_2^30", nullptr, 1, DP, DO, one, h8192, n4096, 32, D, 64, D, 32, 0);
    R(conv2d_winograd36_nhwc_f32, "output_2^29", nullptr, 1, DP, DO, one, n4096, w2048, 32, D, 64, D, 64, 0);
    R(conv2d_winograd36_nhwc_f32_splitk, "input_2^30", nullptr, D, D, 1, 8192, 4096, 32, D, 64, D, 32, 0, 2, D);
    // conv2d_nhwc_bf16(stream, nseg, x, residual, out, batch, height, width, Cin, wpack_hi, wpack_lo, ldw, bias, Cout, KH, KW, stride, pad, relu)
    R(conv2d_nhwc_bf16, "cin_not_32", nullptr, 1, DVP, nullptr, DVO, one, h64, w96, 48, D, nullptr, 64, D, 64, 3, 3, 1, 1, 0);
    R(conv2d_nhwc_bf16, "ldw_below_cout", nullptr, 1, DVP, nullptr, DVO, one, h64, w96, 64, D, nullptr, 32, D, 64, 3, 3, 1, 1, 0);
    R(conv2d_nhwc_bf16, "input_2^30", nullptr, 1, DVP, nullptr, DVO, one, h8192, n4096, 32, D, nullptr, 32, D, 32, 3, 3, 1, 1, 0);
    R(conv2d_nhwc_bf16, "output_2^29", nullptr, 1, DVP, nullptr, DVO, one, n4096, w2048, 32, D, nullptr, 64, D, 64, 1, 1, 1, 0, 0);
    // conv1x1_frag_nhwc_f32(stream, x, residual, out, batch, height, width, Cin, wpack, bias, Cout, stride, relu, residual_up)
    R(conv1x1_frag_nhwc_f32, "cin_not_32", nullptr, D, nullptr, D, 1, 64, 96, 48, D, D, 64, 1, 0, 0);
    R(conv1x1_frag_nhwc_f32, "input_2^30", nullptr, D, nullptr, D, 1, 8192, 4096, 32, D, D, 32, 1, 0, 0);
    R(conv1x1_frag_nhwc_f32, "output_2^29", nullptr, D, nullptr, D, 1, 4096, 2048, 32, D, D, 64, 1, 0, 0);
    R(conv1x1_frag_nhwc_f32_splitk, "input_2^30", nullptr, D, nullptr, D, 1, 8192, 4096, 32, D, D, 32, 1, 0, 2, D);
    R(conv1x1_siblings_nhwc_f32, "input_2^30", nullptr, D, D, D, 1, 8192, 4096, 32, D, D, 32, 32, 1, 0, 0);
    R(conv1x1_ksw_nhwc_f32, "input_huge", nullptr, D, nullptr, D, 1, 32768, 32768, 32, D, D, 32, 1, 0, 0, 0, 0);
    R(conv3x3_ksw_nhwc_f32, "input_huge", nullptr, D, D, 1, 32768, 32768, 32, D, D, 32, 0);
    R(conv1x1_pair_nhwc_f32, "input_huge", nullptr, D, D, D, D, 1L << 31, 64, D, D, 128, D, D, 64);
    // deform_conv_fused_nhwc(stream, nlev, x, offset, mask, out, height, width, cin, cout, kh, kw, pad, stride, dil, wpack, bias, relu)
    R(deform_conv_fused_nhwc, "cin_not_32", nullptr, 1, DP, DP, nullptr, DO, h64, w96, 48, 64, 3, 3, 1, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc, "empty_output", nullptr, 1, DP, DP, nullptr, DO, h2, h2, 64, 64, 5, 5, 0, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc, "input_2^30", nullptr, 1, DP, DP, nullptr, DO, h8192, n4096, 32, 32, 3, 3, 1, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc, "output_2^29", nullptr, 1, DP, DP, nullptr, DO, n4096, w2048, 32, 64, 1, 1, 0, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc_splitk, "input_2^30", nullptr, D, D, nullptr, D, 8192, 4096, 32, 32, 3, 3, 1, 1, 1, D, D, 0, 2, D);
    R(deform_conv_fused_nhwc_bf16, "cin_not_32", nullptr, 1, DP, DP, nullptr, DO, h64, w96, 48, 64, 3, 3, 1, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc_bf16, "input_2^30", nullptr, 1, DP, DP, nullptr, DO, h8192, n4096, 32, 32, 3, 3, 1, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc_bf16, "output_2^29", nullptr, 1, DP, DP, nullptr, DO, n4096, w2048, 32, 64, 1, 1, 0, 1, 1, D, D, 0);
    R(deform_conv_forward_nhwc, "input_2^30", nullptr, 1, DP, DP, nullptr, DO, h8192, n4096, 32, 32, 3, 3, 1, 1, 1, 1, 1, 1, 1, D, 32, D, 0);
    R(deconv2x2_nhwc_f32, "input_2^30", nullptr, D, 1, 8192, 4096, 32, D, 128, D, 32, 0, D);
    R(deconv2x2_frag_nhwc_f32, "input_2^30", nullptr, D, D, 1, 8192, 4096, 32, D, D, 32, 0);
    R(conv2d_stem_nhwc4_f32, "input_huge", nullptr, D, 1, 32768, 32768, D, 64, D, 64, 7, 7, 2, 3, 1, D);
    R(stem_pool_f32, "input_huge", nullptr, D, 1, 32768, 32768, D, D, D);
    // ---- one step inside conv_fill's limits (the launch itself then fails for want of a device: no size refusal)
    R(conv2d_nhwc_f32, "below_limit", nullptr, 1, DP, nullptr, DO, one, h8192, w4095, 32, D, 32, D, 32, 1, 1, 2, 0, 0, 0);       // 2^30 - 2^20 in
    R(conv2d_nhwc_f32, "below_limit", nullptr, 1, DP, nullptr, DO, one, n4096, w2047, 32, D, 64, D, 64, 1, 1, 1, 0, 0, 0);       // 2^29 - 2^18 out
    // ---- the launchers' own, tighter limits: rows that conv_fill lets through (in: 4096 x 2048 x 64 = 2^29 floats exactly)
    R(deform_conv_fused_nhwc, "own_input", nullptr, 1, DP, DP, nullptr, DO, n4096, w2048, 64, 32, 3, 3, 1, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc, "below_limit", nullptr, 1, DP, DP, nullptr, DO, n4096, w2047, 64, 32, 3, 3, 1, 1, 1, D, D, 0);
    R(deform_conv_fused_nhwc_bf16, "own_input", nullptr, 1, DP, DP, nullptr, DO, n4096, w2048, 64, 32, 3, 3, 1, 1, 1, D, D, 0);
    R(conv2d_nhwc_bf16, "own_input", nullptr, 1, DVP, nullptr, DVO, one, n4096, w2048, 64, D, nullptr, 128, D, 32, 3, 3, 1, 1, 0);
    R(conv2d_nhwc_bf16, "below_limit", nullptr, 1, DVP, nullptr, DVO, one, n4096, w2047, 64, D, nullptr, 128, D, 32, 3, 3, 1, 1, 0);
    R(conv1x1_frag_nhwc_f32, "own_input", nullptr, D, nullptr, D, 1, 4096, 2048, 64, D, D, 32, 1, 0, 0);
    R(conv1x1_frag_nhwc_f32, "below_limit", nullptr, D, nullptr, D, 1, 4096, 2047, 64, D, D, 32, 1, 0, 0);
    R(conv1x1_frag_nhwc_f32_splitk, "own_input", nullptr, D, nullptr, D, 1, 4096, 2048, 64, D, D, 32, 1, 0, 2, D);
    R(conv1x1_frag_nhwc_f32_splitk, "own_output", nullptr, D, nullptr, D, 1, 2047, 2049, 64, D, D, 128, 1, 0, 2, D);     // M = 2^22 - 1: only M + a tile passes 2^29 / 128
    R(conv1x1_siblings_nhwc_f32, "own_input", nullptr, D, D, D, 1, 2048, 2048, 128, D, D, 32, 32, 1, 0, 0);
    R(deconv2x2_frag_nhwc_f32, "own_input", nullptr, D, D, 1, 2048, 1024, 256, D, D, 32, 0);
    R(conv2d_winograd_nhwc_f32_tail, "own_input", nullptr, D, D, 2, 1, 2048, 2048, 32, D, 64, D, 32, D, 32, 0);             // 2^28 floats in
    R(bottleneck_bf16, "own_input", nullptr, D, D, 1, 4096, 1024, 64, D, D, D, D, D, D);                                     // 4 * cmid channels: 2^30
    R(bottleneck_bf16, "below_limit", nullptr, D, D, 1, 4096, 1023, 64, D, D, D, D, D, D);
    R(bottleneck_proj_bf16, "own_input", nullptr, D, D, 1, 4096, 2048, 128, 32, 1, D, D, D, D, D, D);
    R(stem_pool_bf16, "own_input", nullptr, D, 1, 16384, 16384, D, D, D);                                                    // 2^28 pixels
    R(stem_pool_bf16, "below_limit", nullptr, D, 1, 16384, 16383, D, D, D);
    R(deconv2x2_nhwc_bf16, "input_2^30", nullptr, D, 1, 8192, 2048, 64, D, 128, D, 32, 0, D, 0);
    // ---- every launcher that takes one image's height and width: 46341 x 46341 >= 2^31 pixels, everything else 1
#define G(name, tag, iv, pv, ...) refuse_gen("upsnet_" #name, tag, upsnet_##name, iv, pv, __VA_ARGS__)
    // (the launchers with no limit on the image size -- ROIAlign, prep_image, mask_paste, seg_term, ... -- have no row)
    G(pq_accumulate, "image_2^31", 1, D, {{3, 46341}, {4, 46341}});
    G(pan_boundary_map, "image_2^31", 1, D, {{4, 46341}, {5, 46341}});
    G(pq_boundary_accumulate, "image_2^31", 1, D, {{4, 46341}, {5, 46341}});
    G(det_eval_image, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(det_eval_boundary_image, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(boundary_masks, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(poly_raster, "image_2^31", 1, D, {{9, 46341}, {10, 46341}});
    G(cs_inst_image, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(cs_pixel_image, "image_2^31", 1, D, {{5, 46341}, {6, 46341}});
    G(pan_format, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_relabel, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(gt_prepare, "image_2^31", 1, D, {{3, 46341}, {4, 46341}});
    G(vis_render, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_vis, "image_2^31", 1, D, {{6, 46341}, {7, 46341}});
    G(cs_inst_expand, "image_2^31", 1, D, {{4, 46341}, {5, 46341}});
    G(pan_track_step, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_track_step_motion, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_stable_colors, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_components, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_absorb, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(pan_segment_scores, "image_2^31", 1, D, {{3, 46341}, {4, 46341}});
    G(pan_score_filter, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    G(video_eval_frame, "image_2^31", 1, D, {{3, 46341}, {4, 46341}});
    G(video_eval_end, "image_2^31", 1, D, {{1, 46341}, {2, 46341}});
    G(mots_eval_frame, "image_2^31", 1, D, {{3, 46341}, {4, 46341}});
    G(mots_eval_end, "image_2^31", 1, D, {{1, 46341}, {2, 46341}});
    G(pan_rle_transitions, "image_2^31", 1, D, {{2, 46341}, {3, 46341}});
    // ... and the ones whose limit is another: an output of 2^40 pixels, a map of 2^30 pixels per sample
    G(restore_label_maps, "image_limit", 1, D, {{7, 1L << 20}, {9, 1L << 20}});
    G(restore_plane_u8, "image_limit", 1, D, {{6, 1L << 20}, {8, 1L << 20}});
    G(group_norm_small_nhwc_f32, "image_limit", 1, D, {{4, 32768}, {5, 32768}, {6, 128}});
    {
        const int one1[1] = {1}, side[1] = {32768};
        report("upsnet_group_norm_nhwc_f32", "image_limit",
               upsnet_group_norm_nhwc_f32(nullptr, 1, DP, DO, one1, side, side, 128, D, D, 1e-5f, 0, nullptr, nullptr, nullptr, 0, D));
    }
#undef G
#undef R
}

int main(int argc, char **argv)
{
    const bool all = argc < 2;
    if (all || !std::strcmp(argv[1], "queries")) queries();
    if (all || !std::strcmp(argv[1], "refusals")) refusals();
    return 0;
}
