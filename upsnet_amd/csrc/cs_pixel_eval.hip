// cs_pixel_eval.hip -- Cityscapes pixel-level IoU / iIoU (the devkit's evalPixelLevelSemanticLabeling), the per-image part: the
// 34 x 34 confusion matrix over label ids, the pixel counts of every ground-truth instance, and the instance-weighted running sums.
// The rules are restated in dataset/cityscapes_pixel_eval.py and DESIGN 4.12; integers only up to the float64 weighting.
//
//   conf int64 [34][34], conf[gt][pred], every pixel counted (ignore-in-eval labels are handled when the scores are formed).
//   inst int [8][1000][3] per image: instance 1000 * label + k of class c (the eight classes of cs_inst_eval.hip) has the cell
//     (c, k) = size | pixels with pred == label | pixels whose pred is an evaluated label of the label's category. Only raw values
//     v > 1000 of the eight classes have a cell; any id an image can hold has one, so nothing is compacted or truncated.
//   wsum double [10][4], rows = the 8 classes, human, vehicle; columns tp | tpWeighted | fn | fnWeighted (running sums).
//   bad int [2]: pixels whose prediction look-up is no label id | pixels whose ground-truth label is above 33 (both left out of
//     every count; the host raises).
// Launches per image (one stream, no host synchronisation): the zero fill of inst; px_tile_kernel; px_weight_kernel.
//   px_tile_kernel   8192 consecutive pixels per workgroup, 16 per lane and step (one 16-byte load of each uint8 map, two of the
//                    uint16 map). One key per pixel = confusion cell | instance cell; the lanes of a wave that hold the same key
//                    add once (ballot + popcount) into an LDS histogram of the matrix and an LDS hash table of the instances the
//                    chunk meets (128 entries; a chunk with more adds the rest to global memory directly); a workgroup adds each
//                    non-zero cell to global memory once.
//   px_weight_kernel one workgroup per row of wsum. The terms of a class's 1000 cells are formed in parallel into LDS, then one
//                    lane adds them to the running sums in ascending instance id (the devkit's order; category rows walk their
//                    classes in ascending label id): sequential on purpose, the order is what makes the sums reproducible.
#include "common.h"
#include "upsnet_hip.h"

#define PX_NL 34
#define PX_CONF (PX_NL * PX_NL)
#define PX_NCLS 8
#define PX_K 1000                       // instance numbers of a class
#define PX_BT 256
#define PX_STEPS 2                      // 16-pixel steps per lane
#define PX_PIX (PX_BT * 16 * PX_STEPS)
#define PX_HASH 128                     // LDS entries for the instances a chunk meets
#define PX_SLOT_SHIFT 11                // key = confusion cell (< 2048) | (instance cell + 1) << 11

typedef unsigned long long px_u64;

struct PxAvg {
    double v[PX_NCLS];
};

// classes 0..7 = person rider car truck bus train motorcycle bicycle = labels 24 25 26 27 28 31 32 33
__device__ static inline int px_label(const int c) { return c < 5 ? 24 + c : 26 + c; }

// cell c * 1000 + k of raw value v in the instance table, -1 for everything that is no instance of the eight classes
__device__ static inline int px_inst_cell(const int v)
{
    if (v <= 1000) return -1;
    const int label = v / 1000;
    int c = -1;
    if (label >= 24 && label <= 28) c = label - 24;
    else if (label >= 31 && label <= 33) c = label - 26;
    if (c < 0) return -1;
    return c * PX_K + (v - 1000 * label);
}

// is prediction label p an evaluated label of the category of class c (human: 24 25; vehicle: 26 27 28 31 32 33)
__device__ static inline bool px_in_category(const int c, const int p)
{
    if (c < 2) return p == 24 || p == 25;
    return (p >= 26 && p <= 28) || (p >= 31 && p <= 33);
}

// One merged group of n pixels with the same key: the matrix cell, and the instance's three counts.
__device__ static inline void px_add_group(int *s_conf, int *s_hkey, int *s_hval, int *__restrict__ inst, const int key, const int n)
{
    const int cell = key & ((1 << PX_SLOT_SHIFT) - 1);
    atomicAdd(&s_conf[cell], n);
    const int slot = (key >> PX_SLOT_SHIFT) - 1;
    if (slot < 0) return;
    const int c = slot / PX_K, p = cell % PX_NL;
    const int n_cls = p == px_label(c) ? n : 0, n_cat = px_in_category(c, p) ? n : 0;
    unsigned h = ((unsigned)slot * 2654435761u) >> 25;      // 7 bits
    for (int probe = 0; probe < PX_HASH; ++probe) {
        const int old = atomicCAS(&s_hkey[h], -1, slot);
        if (old == -1 || old == slot) {
            atomicAdd(&s_hval[3 * h], n);
            if (n_cls) atomicAdd(&s_hval[3 * h + 1], n_cls);
            if (n_cat) atomicAdd(&s_hval[3 * h + 2], n_cat);
            return;
        }
        h = (h + 1) & (PX_HASH - 1);
    }
    // more than PX_HASH distinct instances in this chunk: straight to the table
    atomicAdd(&inst[3 * slot], n);
    if (n_cls) atomicAdd(&inst[3 * slot + 1], n_cls);
    if (n_cat) atomicAdd(&inst[3 * slot + 2], n_cat);
}

__global__ void __launch_bounds__(PX_BT)
px_tile_kernel(const unsigned char *__restrict__ gt_labels, const uint16_t *__restrict__ gt_ids, const unsigned char *__restrict__ pred,
               const unsigned char *__restrict__ lut, const long npix, const bool vec, px_u64 *__restrict__ conf, int *__restrict__ inst,
               int *__restrict__ bad)
{
    __shared__ int s_conf[PX_CONF];
    __shared__ int s_hkey[PX_HASH];
    __shared__ int s_hval[PX_HASH * 3];
    __shared__ unsigned char s_lut[256];
    const int t = threadIdx.x, lane = t & (UPS_WAVE - 1);
    for (int i = t; i < PX_CONF; i += PX_BT) s_conf[i] = 0;
    for (int i = t; i < PX_HASH; i += PX_BT) s_hkey[i] = -1;
    for (int i = t; i < PX_HASH * 3; i += PX_BT) s_hval[i] = 0;
    s_lut[t] = lut[t];
    __syncthreads();
    const long base = (long)blockIdx.x * PX_PIX;
    int bad_pred = 0, bad_gt = 0;
    for (int it = 0; it < PX_STEPS; ++it) {
        const long p0 = base + ((long)it * PX_BT + t) * 16;
        unsigned g[4] = {0u, 0u, 0u, 0u}, q[4] = {0u, 0u, 0u, 0u}, v[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        int valid = 0;
        if (vec && p0 + 16 <= npix) {
            const uint4 a = *(const uint4 *)(gt_labels + p0);
            const uint4 b = *(const uint4 *)(pred + p0);
            g[0] = a.x; g[1] = a.y; g[2] = a.z; g[3] = a.w;
            q[0] = b.x; q[1] = b.y; q[2] = b.z; q[3] = b.w;
            if (gt_ids) {
                const uint4 c0 = *(const uint4 *)(gt_ids + p0);
                const uint4 c1 = *(const uint4 *)(gt_ids + p0 + 8);
                v[0] = c0.x; v[1] = c0.y; v[2] = c0.z; v[3] = c0.w;
                v[4] = c1.x; v[5] = c1.y; v[6] = c1.z; v[7] = c1.w;
            }
            valid = 16;
        } else if (p0 < npix) {
            valid = (int)(npix - p0 < 16 ? npix - p0 : 16);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < valid) {
                    g[i >> 2] |= (unsigned)gt_labels[p0 + i] << (8 * (i & 3));
                    q[i >> 2] |= (unsigned)pred[p0 + i] << (8 * (i & 3));
                    if (gt_ids) v[i >> 1] |= (unsigned)gt_ids[p0 + i] << (16 * (i & 1));
                }
            }
        }
        if (!__ballot(valid != 0)) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int key = -1;
            if (i < valid) {
                const int gl = (g[i >> 2] >> (8 * (i & 3))) & 0xFF;
                const int pl = s_lut[(q[i >> 2] >> (8 * (i & 3))) & 0xFF];
                if (pl >= PX_NL) ++bad_pred;
                else if (gl >= PX_NL) ++bad_gt;
                else key = (gl * PX_NL + pl) | ((px_inst_cell((int)((v[i >> 1] >> (16 * (i & 1))) & 0xFFFFu)) + 1) << PX_SLOT_SHIFT);
            }
            // lanes of equal key add once
            px_u64 act = __ballot(key >= 0);
            while (act) {
                const int leader = __ffsll((long long)act) - 1;
                const int k0 = __builtin_amdgcn_readlane(key, leader);      // (leader comes from a ballot: wave-uniform)
                const px_u64 same = __ballot(key == k0);
                if (lane == leader) px_add_group(s_conf, s_hkey, s_hval, inst, k0, __popcll(same));
                act &= ~same;
            }
        }
    }
    if (bad_pred) atomicAdd(&bad[0], bad_pred);
    if (bad_gt) atomicAdd(&bad[1], bad_gt);
    __syncthreads();
    for (int i = t; i < PX_CONF; i += PX_BT) {
        const int n = s_conf[i];
        if (n) atomicAdd(&conf[i], (px_u64)n);
    }
    if (t < PX_HASH && s_hkey[t] >= 0) {
        const int slot = s_hkey[t];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int n = s_hval[3 * t + j];
            if (n) atomicAdd(&inst[3 * slot + j], n);
        }
    }
}

// rows 0..7: the class itself, column 1 of its cells; row 8: person then rider, row 9: car .. bicycle, column 2 (category)
__global__ void __launch_bounds__(PX_BT)
px_weight_kernel(const int *__restrict__ inst, const PxAvg avg, double *__restrict__ wsum)
{
    __shared__ double s_tpw[PX_K], s_fnw[PX_K];
    __shared__ int s_tp[PX_K], s_fn[PX_K];
    __shared__ px_u64 s_mask[(PX_K + 63) / 64];
    const int row = blockIdx.x, t = threadIdx.x, lane = t & (UPS_WAVE - 1);
    const int c_first = row < PX_NCLS ? row : (row == PX_NCLS ? 0 : 2);
    const int c_last = row < PX_NCLS ? row : (row == PX_NCLS ? 1 : PX_NCLS - 1);
    const int col = row < PX_NCLS ? 1 : 2;
    double tp = 0.0, tpw = 0.0, fn = 0.0, fnw = 0.0;
    if (t == 0) { tp = wsum[4 * row]; tpw = wsum[4 * row + 1]; fn = wsum[4 * row + 2]; fnw = wsum[4 * row + 3]; }
    for (int c = c_first; c <= c_last; ++c) {
        const double a = avg.v[c];
        for (int k0 = 0; k0 < PX_K; k0 += PX_BT) {      // (every lane of a wave takes the same trips: k0 + t is only a bound on the loads)
            const int k = k0 + t;
            int size = 0, hit = 0;
            if (k < PX_K) {
                size = inst[3 * (c * PX_K + k)];
                hit = inst[3 * (c * PX_K + k) + col];
            }
            const px_u64 m = __ballot(size > 0);
            if (size > 0) {
                const double w = a / (double)size;      // the devkit's order: the weight first, then the two products
                s_tpw[k] = (double)hit * w;
                s_fnw[k] = (double)(size - hit) * w;
                s_tp[k] = hit;
                s_fn[k] = size - hit;
            }
            if (lane == 0 && k < PX_K) s_mask[k >> 6] = m;
        }
        __syncthreads();
        if (t == 0) {
            for (int wd = 0; wd < (PX_K + 63) / 64; ++wd) {
                px_u64 m = s_mask[wd];
                while (m) {
                    const int k = wd * 64 + __ffsll((long long)m) - 1;
                    m &= m - 1;
                    tp += (double)s_tp[k];
                    tpw += s_tpw[k];
                    fn += (double)s_fn[k];
                    fnw += s_fnw[k];
                }
            }
        }
        __syncthreads();
    }
    if (t == 0) { wsum[4 * row] = tp; wsum[4 * row + 1] = tpw; wsum[4 * row + 2] = fn; wsum[4 * row + 3] = fnw; }
}

extern "C" size_t upsnet_cs_pixel_inst_ints(void) { return (size_t)PX_NCLS * PX_K * 3; }

extern "C" int upsnet_cs_pixel_image(void *stream, const unsigned char *gt_labels, const uint16_t *gt_ids, const unsigned char *pred,
                                     const unsigned char *lut, int height, int width, const double *avg_class_size, int64_t *conf,
                                     int *inst, double *wsum, int *bad)
{
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * (long)width <= (1L << 30), "cs_pixel_image: map of %d x %d (H * W in 1..2^30)",
                height, width);
    UPS_REQUIRE(gt_labels && pred && lut && conf && bad, "cs_pixel_image: null pointer");
    UPS_REQUIRE(!gt_ids || (inst && wsum && avg_class_size), "cs_pixel_image: an instance-id map needs inst, wsum and avg_class_size");
    UPS_REQUIRE(((uintptr_t)gt_ids & 1) == 0 && ((uintptr_t)conf & 7) == 0 && ((uintptr_t)wsum & 7) == 0 && ((uintptr_t)inst & 3) == 0 &&
                    ((uintptr_t)bad & 3) == 0, "cs_pixel_image: misaligned pointer");
    PxAvg avg;
    for (int c = 0; c < PX_NCLS; ++c) {
        avg.v[c] = gt_ids ? avg_class_size[c] : 1.0;
        UPS_REQUIRE(avg.v[c] > 0.0 && avg.v[c] < 1e300, "cs_pixel_image: average size %g of class %d (must be positive and finite)", avg.v[c], c);
    }
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)height * width;
    if (gt_ids && ups_zero_async(inst, upsnet_cs_pixel_inst_ints() * sizeof(int), st)) return 1;
    const bool vec = (((uintptr_t)gt_labels | (uintptr_t)pred | (uintptr_t)gt_ids) & 15) == 0;
    hipLaunchKernelGGL(px_tile_kernel, dim3((unsigned)ups_divup(npix, PX_PIX)), dim3(PX_BT), 0, st, gt_labels, gt_ids, pred, lut, npix, vec,
                       (px_u64 *)conf, inst, bad);
    UPS_CHECK_LAUNCH("px_tile_kernel");
    if (gt_ids) {
        hipLaunchKernelGGL(px_weight_kernel, dim3(PX_NCLS + 2), dim3(PX_BT), 0, st, (const int *)inst, avg, wsum);
        UPS_CHECK_LAUNCH("px_weight_kernel");
    }
    return 0;
}
