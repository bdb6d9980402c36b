// tta.hip -- the merge step of multi-scale / flip test-time augmentation.
//
// There is no reference implementation (upsnet_end2end_test.py has no augmentation path); DESIGN 4.18 states the rule and
// tests/tta_ref.py restates it in numpy float32. Every kernel here evaluates that rule in fp32 in the written order (the build's
// -ffp-contract=off keeps the products and sums apart), so the device results equal the restatement bit for bit.
//
//   tta_seg_merge_kernel     the A semantic score maps, each bilinearly resampled into the base frame (mirrored for a flipped
//                            augmentation), summed in augmentation order and divided by A: one launch, one store per output element
//   tta_roi_union_kernel     the valid proposal rows of every augmentation, mapped to the base frame and packed behind each other
//                            (device counts, prefix computed in the kernel), with their box deltas and class probabilities
//   tta_boxes_to_aug_kernel  the final boxes mapped from the base frame into every augmentation's frame
//   tta_mask_merge_kernel    the A mask-logit tensors summed in augmentation order (columns mirrored for a flipped one) over A
#include "common.h"
#include "upsnet_hip.h"

#define TTA_MAXA 8

struct TtaSegParams {
    const float *map[TTA_MAXA];
    int hs[TTA_MAXA], ws[TTA_MAXA];
    float q[TTA_MAXA], wr[TTA_MAXA];
    int flip[TTA_MAXA];
    float *out;
    float inv_cell;
    int A, S, Hb, Wb;
};

// V = 4: four channels per lane through 16-byte accesses (S % 4 == 0 and every base 16-byte aligned); V = 1: scalar.
// Lanes run along the channel axis of the channels-last maps: the four corner reads and the store of a wave are contiguous runs.
template <int V>
__global__ void __launch_bounds__(256)
tta_seg_merge_kernel(const TtaSegParams p)
{
    const int nv = p.S / V;
    const long total = (long)p.Hb * p.Wb * nv;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % nv) * V;
    const long pix = idx / nv;
    const int x = (int)(pix % p.Wb), y = (int)(pix / p.Wb);
    float acc[V];
#pragma unroll
    for (int a = 0; a < TTA_MAXA; ++a) {
        if (a >= p.A) break;
        const int Hs = p.hs[a], Ws = p.ws[a];
        const float q = p.q[a];
        const float ty = ((float)y + 0.5f) * q, tx = ((float)x + 0.5f) * q;
        float v = ty - 0.5f;
        float u = p.flip[a] ? (p.wr[a] * p.inv_cell - tx) - 0.5f : tx - 0.5f;
        v = fminf(fmaxf(v, 0.f), (float)(Hs - 1));
        u = fminf(fmaxf(u, 0.f), (float)(Ws - 1));
        const float fy0 = floorf(v), fx0 = floorf(u);
        const float fy = v - fy0, fx = u - fx0;
        // (the float clamp above already bounds the indices; the integer clamp keeps them inside the map whatever q / wr hold)
        const int y0 = min(max((int)fy0, 0), Hs - 1), x0 = min(max((int)fx0, 0), Ws - 1);
        const int y1 = min(y0 + 1, Hs - 1), x1 = min(x0 + 1, Ws - 1);
        const float *m = p.map[a] + c;
        const long S = p.S;
        const float *p00 = m + ((long)y0 * Ws + x0) * S, *p01 = m + ((long)y0 * Ws + x1) * S;
        const float *p10 = m + ((long)y1 * Ws + x0) * S, *p11 = m + ((long)y1 * Ws + x1) * S;
        float m00[V], m01[V], m10[V], m11[V];
        if (V == 4) {
            *reinterpret_cast<float4 *>(m00) = *reinterpret_cast<const float4 *>(p00);
            *reinterpret_cast<float4 *>(m01) = *reinterpret_cast<const float4 *>(p01);
            *reinterpret_cast<float4 *>(m10) = *reinterpret_cast<const float4 *>(p10);
            *reinterpret_cast<float4 *>(m11) = *reinterpret_cast<const float4 *>(p11);
        } else {
            m00[0] = *p00; m01[0] = *p01; m10[0] = *p10; m11[0] = *p11;
        }
        const float gy = 1.0f - fy, gx = 1.0f - fx;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float top = gx * m00[k] + fx * m01[k];
            const float bot = gx * m10[k] + fx * m11[k];
            const float s = gy * top + fy * bot;
            acc[k] = a == 0 ? s : acc[k] + s;
        }
    }
    const float fA = (float)p.A;
    float *o = p.out + (pix * p.S + c);
    if (V == 4) {
        float4 r;
        r.x = acc[0] / fA; r.y = acc[1] / fA; r.z = acc[2] / fA; r.w = acc[3] / fA;
        *reinterpret_cast<float4 *>(o) = r;
    } else {
        *o = acc[0] / fA;
    }
}

extern "C" int upsnet_tta_seg_merge(void *stream, int num_aug, const float *const maps[], const int map_h[], const int map_w[],
                                    const float q[], const float resized_w[], const int flip[], int cell, int num_seg, int height,
                                    int width, float *out)
{
    UPS_REQUIRE(num_aug >= 1 && num_aug <= TTA_MAXA, "tta_seg_merge: 1..%d augmentations (got %d)", TTA_MAXA, num_aug);
    UPS_REQUIRE(maps && map_h && map_w && q && resized_w && flip && out, "tta_seg_merge: null pointer");
    UPS_REQUIRE(num_seg > 0 && height > 0 && width > 0, "tta_seg_merge: non-positive size (%d channels, %dx%d)", num_seg, height, width);
    UPS_REQUIRE(cell == 1 || cell == 4, "tta_seg_merge: cell must be 1 (full resolution) or 4 (quarter resolution), got %d", cell);
    TtaSegParams p;
    bool vec = num_seg % 4 == 0 && ((uintptr_t)out & 15) == 0;
    for (int a = 0; a < TTA_MAXA; ++a) {
        const bool on = a < num_aug;
        UPS_REQUIRE(!on || maps[a], "tta_seg_merge: null pointer (map %d)", a);
        UPS_REQUIRE(!on || (map_h[a] > 0 && map_w[a] > 0), "tta_seg_merge: non-positive size (map %d: %dx%d)", a, on ? map_h[a] : 0,
                    on ? map_w[a] : 0);
        p.map[a] = on ? maps[a] : nullptr;
        p.hs[a] = on ? map_h[a] : 1; p.ws[a] = on ? map_w[a] : 1;
        p.q[a] = on ? q[a] : 1.f; p.wr[a] = on ? resized_w[a] : 0.f; p.flip[a] = on ? (flip[a] != 0) : 0;
        if (on && ((uintptr_t)maps[a] & 15)) vec = false;
    }
    p.out = out; p.inv_cell = 1.0f / (float)cell; p.A = num_aug; p.S = num_seg; p.Hb = height; p.Wb = width;
    const long total = (long)height * width * (vec ? num_seg / 4 : num_seg);
    const dim3 grid((unsigned)((total + 255) / 256));
    if (vec)
        hipLaunchKernelGGL(tta_seg_merge_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(tta_seg_merge_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
    UPS_CHECK_LAUNCH("tta_seg_merge_kernel");
    return 0;
}

// ----------------------------------------------------------------------------------------------- proposal union
struct TtaUnionParams {
    const float *rois[TTA_MAXA], *delta[TTA_MAXA], *prob[TTA_MAXA];
    const int *num[TTA_MAXA];
    float r[TTA_MAXA], wr[TTA_MAXA];
    int flip[TTA_MAXA];
    float *rois_out, *delta_out, *prob_out;
    int *num_out;
    int A, R, D, C;
};

// One thread per output element of the row [rois 5 | delta D | prob C]; every thread recomputes the prefix over the A <= 8 counts
// (wave-uniform loads of at most 8 words that stay in cache: no second launch, no host read).
__global__ void __launch_bounds__(256)
tta_roi_union_kernel(const TtaUnionParams p)
{
    const int rowlen = 5 + p.D + p.C;
    const long total = (long)p.A * p.R * rowlen;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int row = (int)(idx / rowlen), col = (int)(idx % rowlen);
    int src_a = -1, src_row = 0, off = 0;
#pragma unroll
    for (int a = 0; a < TTA_MAXA; ++a) {
        if (a >= p.A) break;
        const int n = min(max(*p.num[a], 0), p.R);
        if (src_a < 0 && row < off + n) { src_a = a; src_row = row - off; }
        off += n;
    }
    if (idx == 0) *p.num_out = off;
    float val = 0.f;
    if (src_a >= 0) {
        const float r = p.r[src_a], wr = p.wr[src_a];
        const bool flip = p.flip[src_a] != 0;
        if (col < 5) {
            const float *b = p.rois[src_a] + (long)src_row * 5;
            if (col == 0) {
                val = 0.f;
            } else if (col == 2) {
                val = r * b[2];
            } else if (col == 4) {
                val = r * b[4] + (r - 1.0f);
            } else {
                float x1 = b[1], x2 = b[3];
                if (flip) {
                    const float w1 = wr - 1.0f;
                    const float x1f = w1 - x2, x2f = w1 - x1;
                    x1 = x1f; x2 = x2f;
                }
                val = col == 1 ? r * x1 : r * x2 + (r - 1.0f);
            }
        } else if (col < 5 + p.D) {
            const int d = col - 5;
            val = p.delta[src_a][(long)src_row * p.D + d];
            if (flip && (d & 3) == 0) val = -val;
        } else {
            val = p.prob[src_a][(long)src_row * p.C + (col - 5 - p.D)];
        }
    }
    if (col < 5)
        p.rois_out[(long)row * 5 + col] = val;
    else if (col < 5 + p.D)
        p.delta_out[(long)row * p.D + (col - 5)] = val;
    else
        p.prob_out[(long)row * p.C + (col - 5 - p.D)] = val;
}

extern "C" int upsnet_tta_roi_union(void *stream, int num_aug, const float *const rois[], const float *const delta[],
                                    const float *const prob[], const int *const num_rois_dev[], const float r[],
                                    const float resized_w[], const int flip[], int capacity, int delta_dim, int num_classes,
                                    float *rois_out, float *delta_out, float *prob_out, int *num_out)
{
    UPS_REQUIRE(num_aug >= 1 && num_aug <= TTA_MAXA, "tta_roi_union: 1..%d augmentations (got %d)", TTA_MAXA, num_aug);
    UPS_REQUIRE(rois && delta && prob && num_rois_dev && r && resized_w && flip && rois_out && delta_out && prob_out && num_out,
                "tta_roi_union: null pointer");
    UPS_REQUIRE(capacity > 0 && delta_dim > 0 && num_classes > 0, "tta_roi_union: non-positive size (capacity %d, %d deltas, %d classes)",
                capacity, delta_dim, num_classes);
    UPS_REQUIRE(delta_dim % 4 == 0, "tta_roi_union: %d box deltas per row is not a multiple of 4", delta_dim);
    UPS_REQUIRE((long)num_aug * capacity <= 8192, "tta_roi_union: %d x %d rows exceed the 8192 the detection selection takes", num_aug, capacity);
    TtaUnionParams p;
    for (int a = 0; a < TTA_MAXA; ++a) {
        const bool on = a < num_aug;
        UPS_REQUIRE(!on || (rois[a] && delta[a] && prob[a] && num_rois_dev[a]), "tta_roi_union: null pointer (augmentation %d)", a);
        p.rois[a] = on ? rois[a] : nullptr; p.delta[a] = on ? delta[a] : nullptr; p.prob[a] = on ? prob[a] : nullptr;
        p.num[a] = on ? num_rois_dev[a] : nullptr;
        p.r[a] = on ? r[a] : 1.f; p.wr[a] = on ? resized_w[a] : 0.f; p.flip[a] = on ? (flip[a] != 0) : 0;
    }
    p.rois_out = rois_out; p.delta_out = delta_out; p.prob_out = prob_out; p.num_out = num_out;
    p.A = num_aug; p.R = capacity; p.D = delta_dim; p.C = num_classes;
    const long total = (long)num_aug * capacity * (5 + delta_dim + num_classes);
    hipLaunchKernelGGL(tta_roi_union_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    UPS_CHECK_LAUNCH("tta_roi_union_kernel");
    return 0;
}

// ----------------------------------------------------------------------------------------------- final boxes -> augmentation frames
struct TtaBoxParams {
    float q[TTA_MAXA], wr[TTA_MAXA];
    int flip[TTA_MAXA];
    const float *boxes;
    float *out;
    int A, n;
};

__global__ void __launch_bounds__(256)
tta_boxes_to_aug_kernel(const TtaBoxParams p)
{
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.A * p.n) return;
    const int a = idx / p.n, i = idx % p.n;
    const float *b = p.boxes + (long)i * 5;
    const float q = p.q[a];
    float x1 = q * b[1], y1 = q * b[2];
    float x2 = q * b[3] + (q - 1.0f), y2 = q * b[4] + (q - 1.0f);
    if (p.flip[a]) {
        const float w1 = p.wr[a] - 1.0f;
        const float x1f = w1 - x2, x2f = w1 - x1;
        x1 = x1f; x2 = x2f;
    }
    float *o = p.out + (long)idx * 5;
    o[0] = b[0]; o[1] = x1; o[2] = y1; o[3] = x2; o[4] = y2;
}

extern "C" int upsnet_tta_boxes_to_aug(void *stream, int num_aug, const float q[], const float resized_w[], const int flip[],
                                       const float *boxes, int num_boxes, float *boxes_out)
{
    UPS_REQUIRE(num_aug >= 1 && num_aug <= TTA_MAXA, "tta_boxes_to_aug: 1..%d augmentations (got %d)", TTA_MAXA, num_aug);
    UPS_REQUIRE(q && resized_w && flip, "tta_boxes_to_aug: null pointer");
    UPS_REQUIRE(num_boxes >= 0 && num_boxes <= (1 << 24), "tta_boxes_to_aug: bad box count %d", num_boxes);
    if (num_boxes == 0) return 0;   // nothing to map (the pointers may be NULL)
    UPS_REQUIRE(boxes && boxes_out, "tta_boxes_to_aug: null pointer");
    TtaBoxParams p;
    for (int a = 0; a < TTA_MAXA; ++a) {
        const bool on = a < num_aug;
        p.q[a] = on ? q[a] : 1.f; p.wr[a] = on ? resized_w[a] : 0.f; p.flip[a] = on ? (flip[a] != 0) : 0;
    }
    p.boxes = boxes; p.out = boxes_out; p.A = num_aug; p.n = num_boxes;
    hipLaunchKernelGGL(tta_boxes_to_aug_kernel, dim3((unsigned)ups_divup((long)num_aug * num_boxes, 256)), dim3(256), 0,
                       (hipStream_t)stream, p);
    UPS_CHECK_LAUNCH("tta_boxes_to_aug_kernel");
    return 0;
}

// ----------------------------------------------------------------------------------------------- mask logits
struct TtaMaskParams {
    const float *in[TTA_MAXA];
    int flip[TTA_MAXA];
    float *out;
    long total;
    int A, C, ms, nhwc;
};

// All inputs and the output share one dense layout: [n][C][ms][ms] (nhwc = 0) or [n][ms][ms][C] (nhwc = 1); one thread per element in
// memory order. A flipped augmentation is read at column ms - 1 - x of the same row, class and plane.
__global__ void __launch_bounds__(256)
tta_mask_merge_kernel(const TtaMaskParams p)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.total) return;
    const int ms = p.ms;
    const long xstride = p.nhwc ? p.C : 1;
    const int x = (int)((idx / xstride) % ms);
    const long mirrored = idx + (long)(ms - 1 - 2 * x) * xstride;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < TTA_MAXA; ++a) {
        if (a >= p.A) break;
        const float v = p.in[a][p.flip[a] ? mirrored : idx];
        acc = a == 0 ? v : acc + v;
    }
    p.out[idx] = acc / (float)p.A;
}

extern "C" int upsnet_tta_mask_merge(void *stream, int num_aug, const float *const logits[], const int flip[], int num_rois,
                                     int num_classes, int mask_size, int nhwc, float *out)
{
    UPS_REQUIRE(num_aug >= 1 && num_aug <= TTA_MAXA, "tta_mask_merge: 1..%d augmentations (got %d)", TTA_MAXA, num_aug);
    UPS_REQUIRE(logits && flip, "tta_mask_merge: null pointer");
    UPS_REQUIRE(num_classes > 0 && mask_size > 0, "tta_mask_merge: non-positive size (%d classes, mask size %d)", num_classes, mask_size);
    UPS_REQUIRE(num_rois >= 0, "tta_mask_merge: bad row count %d", num_rois);
    if (num_rois == 0) return 0;   // nothing to merge (the pointers may be NULL)
    UPS_REQUIRE(out, "tta_mask_merge: null pointer");
    TtaMaskParams p;
    for (int a = 0; a < TTA_MAXA; ++a) {
        const bool on = a < num_aug;
        UPS_REQUIRE(!on || logits[a], "tta_mask_merge: null pointer (augmentation %d)", a);
        p.in[a] = on ? logits[a] : nullptr; p.flip[a] = on ? (flip[a] != 0) : 0;
    }
    p.out = out; p.total = (long)num_rois * num_classes * mask_size * mask_size;
    p.A = num_aug; p.C = num_classes; p.ms = mask_size; p.nhwc = nhwc != 0;
    hipLaunchKernelGGL(tta_mask_merge_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    UPS_CHECK_LAUNCH("tta_mask_merge_kernel");
    return 0;
}
