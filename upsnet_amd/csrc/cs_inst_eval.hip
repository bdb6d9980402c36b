// cs_inst_eval.hip -- Cityscapes instance-level AP (the devkit's evalInstanceLevelSemanticLabeling with its default arguments), the
// per-image part: counts of every predicted mask against the uint16 instance-id map and the match rules per (class, threshold).
// The rules are restated in dataset/cityscapes_eval.py and DESIGN 4.10; integers only up to the two float64 divisions.
//
// A raw map value v is a GT region with labelID = v >= 1000 ? v / 1000 : v. Only regions of the eight instance classes enter the
// metric, and a prediction of class c meets only regions of c, so every table is indexed directly by (class, slot):
//   slot 0 = the group region (v == label id), slot 1 + k = instance v == 1000 * label id + k (k < 1000); CS_SLOTS = 1001.
// Nothing is compacted and nothing has a capacity: whatever ids an image holds, they have a cell. Void is a test on the raw value
// (a 32-bit mask over v < 32), never a table.
//   counts int [n][CS_ROW] = area | void intersection | intersection per slot of the prediction's class, then int [8][CS_SLOTS] GT
//   pixel counts. Zeroed by the launcher, filled through LDS histograms: lanes of a wave that hit the same cell add once
//   (cs_wave_add), a workgroup adds each non-zero cell to global memory once.
// Launches per image (one stream, no host synchronisation):
//   cs_gt_kernel     64 x 64 tiles of the map: GT pixel counts; on request also the transposed copy, on which the column-major runs
//                    of a prediction are contiguous reads (walking the row-major map strided is as fast without it: measured, 4.10)
//   cs_rle_kernel    one wave per run of ones, a prediction's runs dealt round-robin to the waves of its workgroups; only the
//                    prediction's own pixels are read
//   cs_dense_kernel  (dense uint8 masks instead) 16 mask bytes per lane and step, the map read under non-zero bytes only
//   cs_pred_kernel   one wave per prediction: its best-overlapping region (overlap > 0.5 holds for at most one region, as regions
//                    are disjoint and the rounded quotient exceeds 0.5 only if the exact one does) and its ignore pixels
//   cs_match_kernel  one workgroup per (threshold, class): the true positive of every valid GT (largest score, then the first
//                    prediction), a code per prediction (1 = (1, score), 2 = (0, score), 0 = no entry), hard false negatives
#include "common.h"
#include "upsnet_hip.h"

#define CS_NCLS 8
#define CS_SLOTS 1001
#define CS_ROW (CS_SLOTS + 2)           // area, void intersection, slots
#define CS_VOID_SLOT CS_SLOTS           // LDS cell of the void intersection
#define CS_MIN_REGION 100
#define CS_MAX_THR 16
#define CS_MAX_PREDS 65535
#define CS_BT 256
#define CS_NW (CS_BT / UPS_WAVE)
#define CS_RLE_CHUNKS 8                 // workgroups per run-length prediction
#define CS_DENSE_STEPS 4                // 16-byte steps per lane in the dense pass
#define CS_DENSE_PIX (CS_BT * 16 * CS_DENSE_STEPS)
// ignoreInEval labels 0 1 2 3 4 5 6 9 10 14 15 16 18 29 30, as bits
#define CS_VOID_MASK 0x6005C67Fu
// state: hard false negatives [8][CS_MAX_THR] | images with a valid GT [8] | predictions of non-zero area [8]
#define CS_STATE_GT (CS_NCLS * CS_MAX_THR)
#define CS_STATE_PRED (CS_STATE_GT + CS_NCLS)

typedef unsigned long long cs_u64;

struct CsPred {
    double ov;          // largest overlap with a region of the prediction's class (0 if none)
    long long ign;      // void + group + small-region intersections
    int slot;           // that region's slot, -1 if none
    int pad;
};

struct CsThr {
    double v[CS_MAX_THR];
};

// classes 0..7 = person rider car truck bus train motorcycle bicycle = labels 24 25 26 27 28 31 32 33
__device__ static inline int cs_label(const int c) { return c < 5 ? 24 + c : 26 + c; }
__device__ static inline int cs_class_of(const int label)
{
    if (label >= 24 && label <= 28) return label - 24;
    if (label >= 31 && label <= 33) return label - 26;
    return -1;
}

// cell of raw value v in the [8][CS_SLOTS] GT table, -1 for the regions of other labels
__device__ static inline int cs_gt_cell(const int v)
{
    const int label = v >= 1000 ? v / 1000 : v;
    const int c = cs_class_of(label);
    if (c < 0) return -1;
    return c * CS_SLOTS + (v >= 1000 ? 1 + v - 1000 * label : 0);
}

// cell of raw value v for a prediction of label L: its slot, CS_VOID_SLOT, or -1
__device__ static inline int cs_pred_cell(const int v, const int L)
{
    if (v == L) return 0;
    if (v >= 1000 && v / 1000 == L) return 1 + v - 1000 * L;
    if (v < 32 && ((CS_VOID_MASK >> v) & 1u)) return CS_VOID_SLOT;
    return -1;
}

// Every lane of the wave calls this together; lanes with cell >= 0 add one to s_hist[cell], lanes of equal cell as one LDS atomic.
__device__ static inline void cs_wave_add(int *s_hist, const int cell, const int lane)
{
    cs_u64 act = __ballot(cell >= 0);
    while (act) {
        const int leader = __ffsll((long long)act) - 1;
        const int c0 = __shfl(cell, leader, UPS_WAVE);
        const cs_u64 same = __ballot(cell == c0);
        if (lane == leader) atomicAdd(&s_hist[c0], __popcll(same));
        act &= ~same;
    }
}

template <bool TRANSPOSE>
__global__ void __launch_bounds__(CS_BT)
cs_gt_kernel(const uint16_t *__restrict__ gt, const int H, const int W, uint16_t *__restrict__ gt_t, int *__restrict__ gtcnt)
{
    __shared__ int s_hist[CS_NCLS * CS_SLOTS];
    __shared__ uint16_t s_tile[64][66];
    const int t = threadIdx.x, lane = t & (UPS_WAVE - 1), wave = t / UPS_WAVE;
    for (int i = t; i < CS_NCLS * CS_SLOTS; i += CS_BT) s_hist[i] = 0;
    __syncthreads();
    const int x0 = blockIdx.x * 64, y0 = blockIdx.y * 64;
    for (int r = wave; r < 64; r += CS_NW) {
        const int y = y0 + r, x = x0 + lane;
        int cell = -1;
        if (y < H && x < W) {
            const int v = gt[(long)y * W + x];
            if (TRANSPOSE) s_tile[r][lane] = (uint16_t)v;
            cell = cs_gt_cell(v);
        }
        cs_wave_add(s_hist, cell, lane);
    }
    __syncthreads();
    if (TRANSPOSE) {
        for (int r = wave; r < 64; r += CS_NW) {
            const int x = x0 + r, y = y0 + lane;
            if (x < W && y < H) gt_t[(long)x * H + y] = s_tile[lane][r];
        }
    }
    for (int i = t; i < CS_NCLS * CS_SLOTS; i += CS_BT) {
        const int n = s_hist[i];
        if (n) atomicAdd(&gtcnt[i], n);
    }
}

// One workgroup's cells into the prediction's row.
__device__ static inline void cs_flush_row(const int *s_hist, int *row, const int t)
{
    for (int i = t; i <= CS_VOID_SLOT; i += CS_BT) {
        const int n = s_hist[i];
        if (n) atomicAdd(&row[i == CS_VOID_SLOT ? 1 : 2 + i], n);
    }
}

// map = the transposed id map [W][H] (STRIDED: the row-major map [H][W]); trans int [.] with off int [n + 1]: ascending column-major
// positions x * H + y where prediction p's mask changes, the first starting a run of ones
template <bool STRIDED>
__global__ void __launch_bounds__(CS_BT)
cs_rle_kernel(const uint16_t *__restrict__ map, const int H, const int W, const int *__restrict__ cls, const int *__restrict__ trans,
              const int *__restrict__ off, int *__restrict__ counts)
{
    __shared__ int s_hist[CS_SLOTS + 1];
    __shared__ int s_area;
    const int p = blockIdx.y;
    const int c = cls[p];
    if (c < 1 || c > CS_NCLS) return;
    const int L = cs_label(c - 1);
    const int npix = H * W;
    const int t = threadIdx.x, lane = t & (UPS_WAVE - 1), wave = t / UPS_WAVE;
    for (int i = t; i <= CS_VOID_SLOT; i += CS_BT) s_hist[i] = 0;
    if (t == 0) s_area = 0;
    __syncthreads();
    const int t0 = off[p], nt = off[p + 1] - t0;
    const int nruns = (nt + 1) / 2;
    int area = 0;
    for (int k = blockIdx.x * CS_NW + wave; k < nruns; k += gridDim.x * CS_NW) {
        // (a list outside the contract -- not ascending, outside the image -- stays inside the map: both ends are clamped)
        int e = 2 * k + 1 < nt ? trans[t0 + 2 * k + 1] : npix;
        int s = trans[t0 + 2 * k];
        e = __builtin_amdgcn_readfirstlane(min(max(e, 0), npix));
        s = __builtin_amdgcn_readfirstlane(min(max(s, 0), e));
        area += e - s;
        for (int q0 = s; q0 < e; q0 += UPS_WAVE) {
            const int q = q0 + lane;
            int cell = -1;
            if (q < e) {
                const int v = STRIDED ? map[(long)(q % H) * W + q / H] : map[q];
                cell = cs_pred_cell(v, L);
            }
            cs_wave_add(s_hist, cell, lane);
        }
    }
    if (lane == 0 && area) atomicAdd(&s_area, area);
    __syncthreads();
    int *row = counts + (long)p * CS_ROW;
    if (s_area == 0) return;
    cs_flush_row(s_hist, row, t);
    if (t == 0) atomicAdd(&row[0], s_area);
}

// masks uint8 [n][H * W] row-major (non-zero = inside), gt the row-major id map
__global__ void __launch_bounds__(CS_BT)
cs_dense_kernel(const uint16_t *__restrict__ gt, const long npix, const int *__restrict__ cls, const unsigned char *__restrict__ masks,
                const bool vec, int *__restrict__ counts)
{
    __shared__ int s_hist[CS_SLOTS + 1];
    __shared__ int s_area;
    const int p = blockIdx.y;
    const int c = cls[p];
    if (c < 1 || c > CS_NCLS) return;
    const int L = cs_label(c - 1);
    const int t = threadIdx.x, lane = t & (UPS_WAVE - 1);
    for (int i = t; i <= CS_VOID_SLOT; i += CS_BT) s_hist[i] = 0;
    if (t == 0) s_area = 0;
    __syncthreads();
    const unsigned char *plane = masks + (long)p * npix;
    const long base = (long)blockIdx.x * CS_DENSE_PIX;
    int area = 0;
    for (int it = 0; it < CS_DENSE_STEPS; ++it) {
        const long p0 = base + ((long)it * CS_BT + t) * 16;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (vec && p0 + 16 <= npix) {
            const uint4 m = *(const uint4 *)(plane + p0);
            w[0] = m.x; w[1] = m.y; w[2] = m.z; w[3] = m.w;
        } else {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (p0 + i < npix) w[i >> 2] |= (unsigned)plane[p0 + i] << (8 * (i & 3));
        }
        if (!__ballot((w[0] | w[1] | w[2] | w[3]) != 0u)) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int cell = -1;
            if ((w[i >> 2] >> (8 * (i & 3))) & 0xFFu) {
                ++area;
                cell = cs_pred_cell(gt[p0 + i], L);
            }
            cs_wave_add(s_hist, cell, lane);
        }
    }
    if (area) atomicAdd(&s_area, area);
    __syncthreads();
    if (s_area == 0) return;
    int *row = counts + (long)p * CS_ROW;
    cs_flush_row(s_hist, row, t);
    if (t == 0) atomicAdd(&row[0], s_area);
}

__global__ void __launch_bounds__(UPS_WAVE)
cs_pred_kernel(const int *__restrict__ counts, const int n, const int *__restrict__ cls, const float *__restrict__ scores,
               CsPred *__restrict__ pm, float *__restrict__ rec_score, unsigned char *__restrict__ rec_cls, cs_u64 *__restrict__ state)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int c = cls[p];
    const int *row = counts + (long)p * CS_ROW;
    const int area = row[0];
    if (c < 1 || c > CS_NCLS || area <= 0) {       // outside the contract / a mask of no pixels: never scored
        if (lane == 0) {
            pm[p].ov = 0.0; pm[p].ign = 0; pm[p].slot = -1; pm[p].pad = 0;
            rec_score[p] = scores[p];
            rec_cls[p] = 0;
        }
        return;
    }
    const int *gtc = counts + (long)n * CS_ROW + (c - 1) * CS_SLOTS;
    long long ign = 0;
    double best = 0.0;
    int bslot = -1;
    for (int s = lane; s < CS_SLOTS; s += UPS_WAVE) {
        const int it = row[2 + s];
        if (it <= 0) continue;
        const int g = gtc[s];
        if (s == 0) ign += it;
        if (g < CS_MIN_REGION) ign += it;
        const double ov = (double)it / (double)((long long)g + (long long)area - (long long)it);
        if (ov > best) { best = ov; bslot = s; }
    }
    for (int o = UPS_WAVE / 2; o > 0; o >>= 1) {
        ign += __shfl_xor(ign, o, UPS_WAVE);
        const double ob = __shfl_xor(best, o, UPS_WAVE);
        const int os = __shfl_xor(bslot, o, UPS_WAVE);
        if (ob > best || (ob == best && os >= 0 && (bslot < 0 || os < bslot))) { best = ob; bslot = os; }
    }
    if (lane == 0) {
        pm[p].ov = best; pm[p].ign = ign + (long long)row[1]; pm[p].slot = bslot; pm[p].pad = 0;
        rec_score[p] = scores[p];
        rec_cls[p] = (unsigned char)c;
        atomicAdd(&state[CS_STATE_PRED + c - 1], 1ull);
    }
}

__device__ static inline cs_u64 cs_key(const float score, const int p)
{
    return ((cs_u64)ups_float_key(score) << 32) | (cs_u64)(0xFFFFFFFFu - (unsigned)p);
}

__global__ void __launch_bounds__(CS_BT)
cs_match_kernel(const int *__restrict__ counts, const int n, const int *__restrict__ cls, const float *__restrict__ scores,
                const CsPred *__restrict__ pm, const CsThr thr, const int num_thr, unsigned char *__restrict__ rec_code,
                cs_u64 *__restrict__ state)
{
    __shared__ cs_u64 s_best[CS_SLOTS];
    __shared__ int s_fn, s_valid;
    const int ti = blockIdx.x, c = blockIdx.y, t = threadIdx.x;
    const double th = thr.v[ti];
    for (int i = t; i < CS_SLOTS; i += CS_BT) s_best[i] = 0;
    if (t == 0) { s_fn = 0; s_valid = 0; }
    __syncthreads();
    const int *gtc = counts + (long)n * CS_ROW + c * CS_SLOTS;
    for (int p = t; p < n; p += CS_BT) {
        if (cls[p] != c + 1 || counts[(long)p * CS_ROW] <= 0) continue;
        const CsPred m = pm[p];
        if (m.slot >= 1 && m.ov > th && gtc[m.slot] >= CS_MIN_REGION) atomicMax(&s_best[m.slot], cs_key(scores[p], p));
    }
    __syncthreads();
    for (int p = t; p < n; p += CS_BT) {
        if (cls[p] != c + 1) continue;
        const int area = counts[(long)p * CS_ROW];
        int code = 0;
        if (area > 0) {
            const CsPred m = pm[p];
            if (m.slot >= 0 && m.ov > th) {
                // a group or a small region above the threshold: neither true nor false positive
                if (m.slot >= 1 && gtc[m.slot] >= CS_MIN_REGION) code = s_best[m.slot] == cs_key(scores[p], p) ? 1 : 2;
            } else if ((double)m.ign / (double)area <= th) {
                code = 2;
            }
        }
        rec_code[(long)p * num_thr + ti] = (unsigned char)code;
    }
    int fn = 0, valid = 0;
    for (int s = 1 + t; s < CS_SLOTS; s += CS_BT) {
        if (gtc[s] >= CS_MIN_REGION) {
            ++valid;
            if (s_best[s] == 0) ++fn;
        }
    }
    if (fn) atomicAdd(&s_fn, fn);
    if (valid) atomicAdd(&s_valid, valid);
    __syncthreads();
    if (t == 0) {       // (the only writer of these cells in this launch; launches of one evaluator are ordered by its stream)
        state[c * CS_MAX_THR + ti] += (cs_u64)s_fn;
        if (ti == 0 && s_valid) state[CS_STATE_GT + c] += 1ull;
    }
}

static inline size_t cs_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t upsnet_cs_inst_counts_ints(int num_preds)
{
    if (num_preds < 0 || num_preds > CS_MAX_PREDS) return 0;
    return (size_t)num_preds * CS_ROW + (size_t)CS_NCLS * CS_SLOTS;
}

extern "C" size_t upsnet_cs_inst_workspace_bytes(int num_preds)
{
    if (num_preds < 0 || num_preds > CS_MAX_PREDS) return 0;
    return cs_align((size_t)(num_preds > 0 ? num_preds : 1) * sizeof(CsPred));
}

extern "C" int upsnet_cs_inst_state_words(void) { return CS_STATE_PRED + CS_NCLS; }

extern "C" int upsnet_cs_inst_image(void *stream, const uint16_t *gt_ids, int height, int width, int num_preds, const int *pred_cls,
                                    const float *pred_scores, const int *trans, const int *trans_off, const unsigned char *masks,
                                    int walk_strided, uint16_t *gt_t, const double *thresholds, int num_thr, int *counts,
                                    void *workspace, float *rec_score, unsigned char *rec_cls, unsigned char *rec_code, int64_t *state)
{
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * (long)width <= (1L << 30), "cs_inst_image: map of %d x %d (H * W in 1..2^30)",
                height, width);
    UPS_REQUIRE(num_preds >= 0 && num_preds <= CS_MAX_PREDS, "cs_inst_image: %d predictions in one image (0..%d)", num_preds, CS_MAX_PREDS);
    UPS_REQUIRE(num_thr >= 1 && num_thr <= CS_MAX_THR, "cs_inst_image: %d thresholds (1..%d)", num_thr, CS_MAX_THR);
    UPS_REQUIRE(gt_ids && thresholds && counts && workspace && state, "cs_inst_image: null pointer");
    for (int i = 0; i < num_thr; ++i)
        UPS_REQUIRE(thresholds[i] >= 0.5 && thresholds[i] < 1.0, "cs_inst_image: threshold %d = %g outside [0.5, 1): a prediction could match two regions",
                    i, thresholds[i]);
    const bool rle = trans_off != nullptr;
    if (num_preds > 0) {
        UPS_REQUIRE(pred_cls && pred_scores && rec_score && rec_cls && rec_code, "cs_inst_image: null pointer");
        UPS_REQUIRE(rle != (masks != nullptr), "cs_inst_image: give run lengths (trans, trans_off) or dense masks, not both or neither");
        UPS_REQUIRE(!rle || trans, "cs_inst_image: null pointer");
        UPS_REQUIRE(!rle || walk_strided || gt_t, "cs_inst_image: the transposed map needs its buffer (gt_t)");
    }
    UPS_REQUIRE(((uintptr_t)counts & 3) == 0 && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)state & 7) == 0 && ((uintptr_t)gt_ids & 1) == 0 &&
                    ((uintptr_t)gt_t & 1) == 0, "cs_inst_image: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const int n = num_preds;
    const long npix = (long)height * width;
    if (ups_zero_async(counts, upsnet_cs_inst_counts_ints(n) * sizeof(int), st)) return 1;
    int *gtcnt = counts + (size_t)n * CS_ROW;
    const dim3 tiles((unsigned)ups_divup(width, 64), (unsigned)ups_divup(height, 64));
    UPS_REQUIRE(tiles.y <= 65535u, "cs_inst_image: map of %d rows (at most 65535 * 64)", height);
    const bool transpose = n > 0 && rle && !walk_strided;
    if (transpose)
        hipLaunchKernelGGL(cs_gt_kernel<true>, tiles, dim3(CS_BT), 0, st, gt_ids, height, width, gt_t, gtcnt);
    else
        hipLaunchKernelGGL(cs_gt_kernel<false>, tiles, dim3(CS_BT), 0, st, gt_ids, height, width, (uint16_t *)nullptr, gtcnt);
    UPS_CHECK_LAUNCH("cs_gt_kernel");
    if (n > 0) {
        if (rle) {
            const dim3 grid(CS_RLE_CHUNKS, (unsigned)n);
            if (transpose)
                hipLaunchKernelGGL(cs_rle_kernel<false>, grid, dim3(CS_BT), 0, st, (const uint16_t *)gt_t, height, width, pred_cls, trans, trans_off, counts);
            else
                hipLaunchKernelGGL(cs_rle_kernel<true>, grid, dim3(CS_BT), 0, st, gt_ids, height, width, pred_cls, trans, trans_off, counts);
            UPS_CHECK_LAUNCH("cs_rle_kernel");
        } else {
            const bool vec = ((uintptr_t)masks & 15) == 0 && (npix & 15) == 0;
            hipLaunchKernelGGL(cs_dense_kernel, dim3((unsigned)ups_divup(npix, CS_DENSE_PIX), (unsigned)n), dim3(CS_BT), 0, st, gt_ids, npix, pred_cls,
                               masks, vec, counts);
            UPS_CHECK_LAUNCH("cs_dense_kernel");
        }
        hipLaunchKernelGGL(cs_pred_kernel, dim3((unsigned)n), dim3(UPS_WAVE), 0, st, (const int *)counts, n, pred_cls, pred_scores, (CsPred *)workspace,
                           rec_score, rec_cls, (cs_u64 *)state);
        UPS_CHECK_LAUNCH("cs_pred_kernel");
    }
    CsThr thr;
    for (int i = 0; i < CS_MAX_THR; ++i) thr.v[i] = i < num_thr ? thresholds[i] : 2.0;
    hipLaunchKernelGGL(cs_match_kernel, dim3((unsigned)num_thr, CS_NCLS), dim3(CS_BT), 0, st, (const int *)counts, n, pred_cls, pred_scores,
                       (const CsPred *)workspace, thr, num_thr, rec_code, (cs_u64 *)state);
    UPS_CHECK_LAUNCH("cs_match_kernel");
    return 0;
}
