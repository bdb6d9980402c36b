// box_vote.hip -- score-weighted box voting on the detection selection's output (gfx950), DESIGN.md 4.21.
//
// The selection (detect.hip) keeps one box per NMS cluster and drops the other candidates of the cluster. With test-time augmentation
// (tta.hip) those candidates are the decodes of the same object from every scale and mirror; voting replaces each kept box by the
// score-weighted mean of the candidates of its class that overlap it (Detectron's TEST.BBOX_VOTE with `ID` scoring: scores, classes and
// order stay). The reference has no voting, so the rule is this project's own and is stated in include/upsnet_hip.h; the sums have one
// fixed order (64 stripes in ascending row order, then a fixed tree), which is one wavefront walking the candidate rows with lane j
// and a shuffle-down reduction, so the result is bit-identical to the numpy restatement (tests/box_vote_ref.py).
//
// One wave64 per kept row, BV_T / 64 rows per workgroup, waves stride over the kept rows; no LDS, no atomics. The candidate of (row r,
// class c) is decoded again from rois / delta with ups_decode_clip, exactly as mroi_candidates_kernel built it, and only for rows that
// pass the score test (the decode costs two fp64 exps). prob[r, c] is a strided 4-byte gather: BV_U iterations' loads are issued
// before the first threshold test.
#include "common.h"
#include "upsnet_hip.h"

#define BV_T 256   // 4 waves
#define BV_U 8     // rows per lane whose probabilities are in flight together
#define BV_MAX_BLOCKS 512

__global__ void __launch_bounds__(BV_T)
box_vote_kernel(const float *__restrict__ rois, const float *__restrict__ delta, const float *__restrict__ prob, const int num_rois,
                const int *__restrict__ num_rois_dev, const int C, const float *__restrict__ im_info, const int clip, const float wx,
                const float wy, const float ww, const float wh, const float score_thresh, const float iou_thresh,
                const float *__restrict__ boxes, const int64_t *__restrict__ cls, const int *__restrict__ num, const int cap,
                float *__restrict__ voted)
{
    const int lane = threadIdx.x & 63;
    // wave w of workgroup g takes rows w * gridDim.x + g, ...: a short kept list spreads over the workgroups, one wave each
    const int wave = (threadIdx.x >> 6) * gridDim.x + blockIdx.x, waves = gridDim.x * (BV_T / 64);
    const int n = min(max(num_rois_dev ? *num_rois_dev : num_rois, 0), num_rois);
    const int kn = min(max(*num, 0), cap);      // (a negative count is the selection's overflow marker: every row is copied)
    const float im_h = im_info[0], im_w = im_info[1];
    for (int k = wave; k < kn; k += waves) {    // (wave-uniform: every lane of a wave reaches the shuffles below)
        const int c = (int)min(max(cls[k], (int64_t)0), (int64_t)(C - 1));
        const float *b = boxes + (long)k * 5;
        const float b0 = b[0], bx1 = b[1], by1 = b[2], bx2 = b[3], by2 = b[4];
        const float *pc = prob + c, *dc = delta + 4 * c;
        float sw = 0.f, sx1 = 0.f, sy1 = 0.f, sx2 = 0.f, sy2 = 0.f;     // stripe `lane`: rows lane, lane + 64, ... in ascending order
        for (int r0 = lane; r0 < n; r0 += 64 * BV_U) {
            float w[BV_U];
#pragma unroll
            for (int u = 0; u < BV_U; ++u) {
                const int r = r0 + 64 * u;
                w[u] = r < n ? pc[(long)r * C] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < BV_U; ++u) {
                const int r = r0 + 64 * u;
                if (r < n && w[u] > score_thresh) {
                    const float *rr = rois + (long)r * 5;
                    const float *d = dc + (long)r * 4 * C;
                    float o[4];
                    ups_decode_clip(rr[1], rr[2], rr[3], rr[4], d[0], d[1], d[2], d[3], wx, wy, ww, wh, im_h, im_w, clip != 0, o);
                    if (ups_iou(bx1, by1, bx2, by2, o[0], o[1], o[2], o[3]) >= iou_thresh) {     // (a NaN IoU is not a voter)
                        sw = sw + w[u];
                        sx1 = sx1 + w[u] * o[0];     // one rounded multiply, one rounded add (-ffp-contract=off)
                        sy1 = sy1 + w[u] * o[1];
                        sx2 = sx2 + w[u] * o[2];
                        sy2 = sy2 + w[u] * o[3];
                    }
                }
            }
        }
        // p[j] = p[j] + p[j + s] for j < s, s = 32 .. 1: lane 0 ends with the stated tree (the lanes >= s compute values nobody reads)
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            sw = sw + __shfl_down(sw, s, 64);
            sx1 = sx1 + __shfl_down(sx1, s, 64);
            sy1 = sy1 + __shfl_down(sy1, s, 64);
            sx2 = sx2 + __shfl_down(sx2, s, 64);
            sy2 = sy2 + __shfl_down(sy2, s, 64);
        }
        if (lane == 0) {
            float x1 = bx1, y1 = by1, x2 = bx2, y2 = by2;
            if (sw > 0.f) {
                x1 = sx1 / sw; y1 = sy1 / sw; x2 = sx2 / sw; y2 = sy2 / sw;
                if (clip) {     // a rounded weighted mean may leave the clipped range by an ulp
                    const float w1 = im_w - 1.0f, h1 = im_h - 1.0f;
                    x1 = fmaxf(fminf(x1, w1), 0.f);
                    y1 = fmaxf(fminf(y1, h1), 0.f);
                    x2 = fmaxf(fminf(x2, w1), 0.f);
                    y2 = fmaxf(fminf(y2, h1), 0.f);
                }
            }
            float *o = voted + (long)k * 5;
            o[0] = b0; o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
        }
    }
    // rows [kn, cap): a bit copy (the selection's zero rows past the count stay zero for the fixed-capacity consumers)
    const uint32_t *src = reinterpret_cast<const uint32_t *>(boxes);
    uint32_t *dst = reinterpret_cast<uint32_t *>(voted);
    const long total = (long)cap * 5;
    for (long i = (long)kn * 5 + (long)blockIdx.x * BV_T + threadIdx.x; i < total; i += (long)gridDim.x * BV_T) dst[i] = src[i];
}

extern "C" int upsnet_box_vote(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                               const int *num_rois_dev, int num_classes, const float *im_info, int clip_boxes,
                               const float reg_weights[4], float vote_score_thresh, float vote_iou_thresh, const float *boxes,
                               const int64_t *cls, const int *num, int cap, float *voted)
{
    UPS_REQUIRE(rois && bbox_delta && cls_prob && im_info && reg_weights && num, "box_vote: null pointer");
    UPS_REQUIRE(num_rois >= 1 && num_rois <= (1 << 24) && num_classes >= 2,
                "box_vote: need 1..2^24 rois and at least two classes (got %d rois, %d classes)", num_rois, num_classes);
    UPS_REQUIRE(cap >= 0 && cap <= (1 << 28), "box_vote: bad capacity %d", cap);
    UPS_REQUIRE(vote_iou_thresh > 0.f, "box_vote: the IoU threshold must be positive (got %g)", (double)vote_iou_thresh);   // (NaN fails too)
    if (cap == 0) return 0;     // nothing to vote or copy (boxes / cls / voted may be NULL)
    UPS_REQUIRE(boxes && cls && voted, "box_vote: null pointer");
    const int need = ups_divup(cap, BV_T / 64), blocks = need < BV_MAX_BLOCKS ? need : BV_MAX_BLOCKS;
    hipLaunchKernelGGL(box_vote_kernel, dim3(blocks), dim3(BV_T), 0, (hipStream_t)stream, rois, bbox_delta, cls_prob, num_rois,
                       num_rois_dev, num_classes, im_info, clip_boxes, reg_weights[0], reg_weights[1], reg_weights[2], reg_weights[3],
                       vote_score_thresh, vote_iou_thresh, boxes, cls, num, cap, voted);
    UPS_CHECK_LAUNCH("box_vote_kernel");
    return 0;
}
