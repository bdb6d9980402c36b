// detect.hip -- detection selection (MaskROI) entirely on the device (gfx950).
//
// Reference: upsnet/operators/modules/mask_roi.py:36-146 copies rois / deltas / probabilities to the
// host, decodes in numpy, loops over classes calling gpu_nms (malloc + H2D + D2H each) and builds the
// result on the host. Here: one launch builds every class's candidate list in ROI order (ordered
// compaction with wave scans), the batched NMS of nms.hip resolves all classes at once, and one
// workgroup applies the global top-max_det rule (radix select of the max_det-th largest score, `>=`
// keep, order preserved) and writes the result, including the reference's dummy ROI when empty.
#include "common.h"
#include "soft_nms_trips.h"
#include "sort.h"
#include "upsnet_hip.h"

int ups_nms_batched_impl(hipStream_t st, const float *boxes, const float *scores, const int *counts,
                         const uint8_t *pre_removed, int P, int nmax, float thresh, int tie_mode, int *keep_idx,
                         int *keep_cnt, void *workspace, int ge);

#define DET_T 1024

// exclusive scan of a 0/1 flag over the workgroup; returns offset, total via *total
__device__ static inline int det_block_scan(int v, int *sh, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(v != 0);
    const int within = __builtin_popcountll(bal & ((1ULL << lane) - 1ULL));
    if (lane == 0) sh[wave] = __builtin_popcountll(bal);
    __syncthreads();
    int base = 0, tot = 0;
    for (int w = 0; w < DET_T / 64; ++w) { const int c = sh[w]; if (w < wave) base += c; tot += c; }
    __syncthreads();
    *total = tot;
    return base + within;
}

#define MROI_FILL 256   // rows of the output buffers that are always defined (zero boxes past the count)

// problem p: class j = p+1 (class-wise) or the single class-agnostic problem.
__global__ void __launch_bounds__(DET_T)
mroi_candidates_kernel(const float *__restrict__ rois, const float *__restrict__ delta, const float *__restrict__ prob,
                       const int num_rois, const int *__restrict__ num_rois_dev, const int C, const float *__restrict__ im_info,
                       const int class_agnostic, const int clip, const float score_thresh, const float wx, const float wy,
                       const float ww, const float wh, const int nmax, float *__restrict__ cboxes, float *__restrict__ cscores,
                       int *__restrict__ csrc, int *__restrict__ ccls, int *__restrict__ counts, int *__restrict__ status)
{
    __shared__ int sh[DET_T / 64];
    const int p = blockIdx.x;
    const int N = num_rois_dev ? min(*num_rois_dev, num_rois) : num_rois;
    const float im_h = im_info[0], im_w = im_info[1];
    const long total = class_agnostic ? (long)N * (C - 1) : N;
    int cnt = 0;
    bool overflow = false;
    for (long base = 0; base < total; base += DET_T) {
        const long q = base + threadIdx.x;
        int r = 0, c = 0;
        float s = 0.f;
        bool flag = false;
        if (q < total) {
            if (class_agnostic) { r = (int)(q / (C - 1)); c = (int)(q % (C - 1)) + 1; } else { r = (int)q; c = p + 1; }
            s = prob[(long)r * C + c];
            flag = s > score_thresh;
        }
        int tot;
        const int pos = cnt + det_block_scan(flag, sh, &tot);
        if (flag) {
            if (pos < nmax) {
                const float *rr = rois + (long)r * 5;
                const float *d = delta + (long)r * 4 * C + 4 * c;
                float o[4];
                ups_decode_clip(rr[1], rr[2], rr[3], rr[4], d[0], d[1], d[2], d[3], wx, wy, ww, wh, im_h, im_w, clip != 0, o);
                float *b = cboxes + ((long)p * nmax + pos) * 4;
                b[0] = o[0]; b[1] = o[1]; b[2] = o[2]; b[3] = o[3];
                cscores[(long)p * nmax + pos] = s;
                csrc[(long)p * nmax + pos] = r;
                ccls[(long)p * nmax + pos] = c;
            } else {
                overflow = true;
            }
        }
        cnt += tot;
    }
    if (overflow) atomicOr(status, 1);
    if (threadIdx.x == 0) counts[p] = min(cnt, nmax);
}

// r11: FLATTENED. The kept detections of all classes form one list in (class, NMS order) -- entry j belongs to the class whose prefix
// range contains j. r03-r10 walked the classes one after the other in each of the four radix passes and again in the compaction, two
// dependent global loads (keep_idx -> score) per class and pass: ~45 us for 8 classes, P x that for 80. Now every thread gathers its
// entries' score keys ONCE into LDS (all loads of a thread in flight together), the radix select of the max_det-th largest score runs on
// the LDS copy, and the ordered compaction walks the flat list in chunks of 1024 (one or two chunks instead of P).
__global__ void __launch_bounds__(DET_T)
mroi_finalize_kernel(const int P, const int nmax, const int max_det, const float *__restrict__ cboxes,
                     const float *__restrict__ cscores, const int *__restrict__ csrc, const int *__restrict__ ccls,
                     const int *__restrict__ keep_idx, const int *__restrict__ keep_cnt, float *__restrict__ boxes_out,
                     float *__restrict__ scores_out, int64_t *__restrict__ cls_out, int *__restrict__ src_out,
                     int *__restrict__ num_out, const int *__restrict__ status, unsigned *__restrict__ flat_keys_g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    int *s_start = reinterpret_cast<int *>(smem_raw);                  // [P + 1] first flat index of every class
    __shared__ int sh[DET_T / 64];
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_need;
    const int tid = threadIdx.x;
    if (tid == 0) { int t = 0; for (int p = 0; p < P; ++p) { s_start[p] = t; t += min(keep_cnt[p], nmax); } s_start[P] = t; }
    __syncthreads();
    const int T = s_start[P];
    // flat entry j -> (class p, position i): binary search in the prefix table
#define MROI_LOCATE(J, PP, II) { int lo_ = 0, hi_ = P; while (hi_ - lo_ > 1) { const int mid_ = (lo_ + hi_) >> 1; if (s_start[mid_] <= (J)) lo_ = mid_; else hi_ = mid_; } \
        PP = lo_; II = (J) - s_start[lo_]; }
    // ---- image_thresh = sorted(all kept scores)[-max_det]  (mask_roi.py:109-111), via MSB radix select on the gathered keys
    unsigned thr_key = 0;  // keep everything by default
    if (max_det > 0 && T > max_det) {
        for (int j = tid; j < T; j += DET_T) {
            int p, i;
            MROI_LOCATE(j, p, i)
            flat_keys_g[j] = ups_float_key(cscores[(long)p * nmax + keep_idx[(long)p * nmax + i]]);
        }
        if (tid == 0) { s_prefix = 0; s_need = (unsigned)max_det; }
        __syncthreads();     // (the keys written above are read back by other threads of this workgroup)
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            for (int i = tid; i < 256; i += DET_T) hist[i] = 0;
            __syncthreads();
            const unsigned prefix = s_prefix;
            const unsigned himask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
            for (int j = tid; j < T; j += DET_T) {
                const unsigned k = flat_keys_g[j];
                if ((k & himask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1u);
            }
            __syncthreads();
            // the bin that holds the need-th largest key: thread b < 256 owns bin b and sums the bins above it (255 independent broadcast
            // LDS reads; r03-r10: ONE thread walked the bins downwards, a dependent LDS read per bin -- ~8 us per pass, 4 passes)
            const unsigned need0 = s_need;
            __syncthreads();
            if (tid < 256) {
                unsigned above = 0;
                for (int u = tid + 1; u < 256; ++u) above += hist[u];
                const unsigned v = hist[tid];
                // largest b with (sum of the bins above b) < need <= that sum + hist[b]; if no bin reaches `need` the walk ended at b = 0
                if (above < need0 && (need0 <= above + v || tid == 0)) {
                    s_prefix = prefix | ((unsigned)tid << shift);
                    s_need = need0 - above;
                }
            }
            __syncthreads();
        }
        thr_key = s_prefix;
    }
    // ---- ordered compaction over the flat list = (class, NMS order)
    int cnt = 0;
    for (int base = 0; base < T; base += DET_T) {
        const int j = base + tid;
        int src = 0, p = 0;
        float s = 0.f;
        bool flag = false;
        if (j < T) {
            int i;
            MROI_LOCATE(j, p, i)
            src = keep_idx[(long)p * nmax + i];
            s = cscores[(long)p * nmax + src];
            flag = ups_float_key(s) >= thr_key;
        }
        int tot;
        const int pos = cnt + det_block_scan(flag, sh, &tot);
        if (flag) {
            const float *b = cboxes + ((long)p * nmax + src) * 4;
            float *o = boxes_out + (long)pos * 5;
            o[0] = 0.f; o[1] = b[0]; o[2] = b[1]; o[3] = b[2]; o[4] = b[3];
            scores_out[pos] = s;
            cls_out[pos] = ccls[(long)p * nmax + src];
            src_out[pos] = csrc[(long)p * nmax + src];
        }
        cnt += tot;
    }
#undef MROI_LOCATE
    // rows [cnt, max(max_det, MROI_FILL)) are defined (zero boxes): callers may run fixed-size work (the mask head inside the HIP graph) on
    // the first max_det rows without reading the counter first
    for (int i = max(cnt, 1) + tid; i < max(max_det, MROI_FILL) && i < P * nmax; i += DET_T) {
        for (int q = 0; q < 5; ++q) boxes_out[(long)i * 5 + q] = 0.f;
        scores_out[i] = 0.f; cls_out[i] = 0; src_out[i] = -1;
    }
    if (tid == 0) {
        if (cnt == 0) {  // mask_roi.py:135-141
            for (int q = 0; q < 5; ++q) boxes_out[q] = 0.f;
            scores_out[0] = 1.f; cls_out[0] = 0; src_out[0] = 0;
            cnt = 1;
        }
        // more candidates than the fixed capacity (class-agnostic mode: 8192) were above the score threshold: the result would
        // silently differ from the reference -- report it through the count (negative), the host raises
        *num_out = *status ? -cnt : cnt;
    }
}

static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }

static void mroi_dims(int N, int C, int agn, int *P, int *nmax)
{
    if (agn) { *P = 1; long m = (long)N * (C - 1); *nmax = (int)(m < 8192 ? (m < 1 ? 1 : m) : 8192); }
    else { *P = C - 1; *nmax = N < 1 ? 1 : N; }
}

extern "C" int upsnet_mask_roi_capacity(int N, int C, int agn)
{
    if (C < 2) return 0;                          // no foreground class: no capacity (never a negative one)
    int P, nmax;
    mroi_dims(N, C, agn, &P, &nmax);
    const long cap = (long)P * nmax;
    return cap > 0x7fffffffL ? 0 : (int)cap;     // beyond an int: no capacity (the launcher's row indices are ints)
}

struct MroiPlan { size_t boxes, scores, src, cls, counts, keep, keepcnt, status, flat, nms, total; };
static MroiPlan mroi_plan(int P, int nmax)
{
    MroiPlan m; size_t o = 0;
    m.boxes = o; o += al256((size_t)P * nmax * 16);
    m.scores = o; o += al256((size_t)P * nmax * 4);
    m.src = o; o += al256((size_t)P * nmax * 4);
    m.cls = o; o += al256((size_t)P * nmax * 4);
    m.counts = o; o += al256((size_t)P * 4);
    m.keep = o; o += al256((size_t)P * nmax * 4);
    m.keepcnt = o; o += al256((size_t)P * 4);
    m.status = o; o += 256;
    m.flat = o; o += al256((size_t)P * nmax * 4);      // score keys of the kept detections, flat (mroi_finalize_kernel)
    m.nms = o; o += upsnet_nms_workspace_bytes(P, nmax);
    m.total = o + 256;
    return m;
}

extern "C" size_t upsnet_mask_roi_workspace_bytes(int N, int C, int agn)
{
    if (N < 1 || C < 2) return 256;                // (what upsnet_mask_roi_ex refuses: no negative problem count reaches the plan)
    int P, nmax;
    mroi_dims(N, C, agn, &P, &nmax);
    return mroi_plan(P, nmax).total;
}

// clip_boxes = 0: MaskROI(clip_boxes=False) (mask_roi.py:53-54 skipped): the decoded boxes go to the NMS unclipped
extern "C" int upsnet_mask_roi_ex(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                                  const int *num_rois_dev, int num_classes, const float *im_info, int class_agnostic, int clip_boxes,
                                  float score_thresh, float nms_thresh, int max_det, const float reg_weights[4],
                                  float *boxes_out, float *scores_out, int64_t *cls_out, int *src_out, int *num_out,
                                  void *workspace)
{
    UPS_REQUIRE(rois && bbox_delta && cls_prob && im_info && reg_weights && boxes_out && scores_out && cls_out && src_out &&
                    num_out && workspace, "mask_roi: null pointer");
    UPS_REQUIRE(num_rois >= 1 && num_classes >= 2, "mask_roi: need at least one roi and two classes");
    int P, nmax;
    mroi_dims(num_rois, num_classes, class_agnostic, &P, &nmax);
    UPS_REQUIRE(nmax <= 8192, "mask_roi: %d candidates per class exceed the 8192 supported", nmax);
    const MroiPlan m = mroi_plan(P, nmax);
    unsigned char *ws = (unsigned char *)workspace;
    float *cboxes = (float *)(ws + m.boxes), *cscores = (float *)(ws + m.scores);
    int *csrc = (int *)(ws + m.src), *ccls = (int *)(ws + m.cls), *counts = (int *)(ws + m.counts);
    int *keep = (int *)(ws + m.keep), *keepcnt = (int *)(ws + m.keepcnt), *status = (int *)(ws + m.status);
    hipStream_t st = (hipStream_t)stream;
    if (ups_zero_async(status, sizeof(int), st)) return 1;
    hipLaunchKernelGGL(mroi_candidates_kernel, dim3(P), dim3(DET_T), 0, st, rois, bbox_delta, cls_prob, num_rois, num_rois_dev,
                       num_classes, im_info, class_agnostic, clip_boxes, score_thresh, reg_weights[0], reg_weights[1], reg_weights[2],
                       reg_weights[3], nmax, cboxes, cscores, csrc, ccls, counts, status);
    UPS_CHECK_LAUNCH("mroi_candidates_kernel");
    int rc = ups_nms_batched_impl(st, cboxes, cscores, counts, nullptr, P, nmax, nms_thresh, 0, keep, keepcnt, ws + m.nms, 0);
    if (rc) return rc;
    hipLaunchKernelGGL(mroi_finalize_kernel, dim3(1), dim3(DET_T), (size_t)(P + 1) * sizeof(int), st, P, nmax, max_det, cboxes, cscores, csrc, ccls, keep,
                       keepcnt, boxes_out, scores_out, cls_out, src_out, num_out, status, (unsigned *)(ws + m.flat));
    UPS_CHECK_LAUNCH("mroi_finalize_kernel");
    return 0;
}

extern "C" int upsnet_mask_roi(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                               const int *num_rois_dev, int num_classes, const float *im_info, int class_agnostic,
                               float score_thresh, float nms_thresh, int max_det, const float reg_weights[4],
                               float *boxes_out, float *scores_out, int64_t *cls_out, int *src_out, int *num_out,
                               void *workspace)
{
    return upsnet_mask_roi_ex(stream, rois, bbox_delta, cls_prob, num_rois, num_rois_dev, num_classes, im_info, class_agnostic, 1,
                              score_thresh, nms_thresh, max_det, reg_weights, boxes_out, scores_out, cls_out, src_out, num_out,
                              workspace);
}

// ---------------------------------------------------------------------------------------------
// Soft detection selection (Detectron's TEST.SOFT_NMS on the class-wise selection). ONE workgroup per class builds the
// class's candidate list in ROI order straight into the LDS structure-of-arrays of the soft-NMS (decode on the fly, ordered compaction
// with ballots), runs the sequential trips there (snms_lds_trips, the body soft_nms_lds_kernel runs) and writes the survivors -- box,
// DECAYED score, source row, class -- compacted at rows 0..N'-1 of the class's workspace slice with an identity keep list, so that
// mroi_finalize_kernel applies the top-max_det rule, the dummy row, the zero fill and the overflow marker exactly as on the hard path.
// A class holds at most SNMS_LDS_MAX candidates (its state is LDS-resident): a class with more keeps its first SNMS_LDS_MAX and sets
// the status word, which the finalize turns into a negative count. T = 64 up to 1024 rows (no real barriers), 256 above.
template <int T>
__global__ void __launch_bounds__(T)
mroi_soft_kernel(const float *__restrict__ rois, const float *__restrict__ delta, const float *__restrict__ prob, const int num_rois,
                 const int *__restrict__ num_rois_dev, const int C, const float *__restrict__ im_info, const int clip,
                 const float score_thresh, const float wx, const float wy, const float ww, const float wh, const int nmax,
                 const int cap, const float sigma, const float Nt, const float floor_thresh, const int method,
                 float *__restrict__ cboxes, float *__restrict__ cscores, int *__restrict__ csrc, int *__restrict__ ccls,
                 int *__restrict__ keep_idx, int *__restrict__ keep_cnt, int *__restrict__ status)
{
    constexpr int W = T / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ SnmsScratch<T> scratch;
    __shared__ int s_cnt[W];
    const SnmsState s = snms_carve(smem_raw, cap);
    const int p = blockIdx.x, c = p + 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int N = min(max(num_rois_dev ? *num_rois_dev : num_rois, 0), num_rois);
    const int limit = min(nmax, SNMS_LDS_MAX);      // (<= cap)
    const float im_h = im_info[0], im_w = im_info[1];
    // ---- 1. the class's candidates, rows ascending, into the LDS state
    int cnt = 0;
    bool overflow = false;
    for (int base = 0; base < N; base += T) {
        const int r = base + tid;
        float sc = 0.f;
        bool flag = false;
        if (r < N) { sc = prob[(long)r * C + c]; flag = sc > score_thresh; }
        const unsigned long long bal = __ballot(flag);
        int pos = cnt + __builtin_popcountll(bal & ((1ULL << lane) - 1ULL)), tot = __builtin_popcountll(bal);
        if (W > 1) {
            if (lane == 0) s_cnt[wave] = tot;
            __syncthreads();
            tot = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) { const int v = s_cnt[w]; if (w < wave) pos += v; tot += v; }
            __syncthreads();
        }
        if (flag) {
            if (pos < limit) {
                const float *rr = rois + (long)r * 5;
                const float *d = delta + (long)r * 4 * C + 4 * c;
                float o[4];
                ups_decode_clip(rr[1], rr[2], rr[3], rr[4], d[0], d[1], d[2], d[3], wx, wy, ww, wh, im_h, im_w, clip != 0, o);
                s.x1[pos] = o[0]; s.y1[pos] = o[1]; s.x2[pos] = o[2]; s.y2[pos] = o[3]; s.sc[pos] = sc;
                s.ind[pos] = r;
            } else {
                overflow = true;
            }
        }
        cnt += tot;
    }
    if (overflow) atomicOr(status, 1);
    __syncthreads();
    // ---- 2. the trips
    const int kept = snms_lds_trips<T>(s, scratch, min(cnt, limit), sigma, Nt, floor_thresh, method);
    // ---- 3. survivors in the reference's order, identity keep list
    const long row0 = (long)p * nmax;
    for (int q = tid; q < kept; q += T) {
        float *b = cboxes + (row0 + q) * 4;
        b[0] = s.x1[q]; b[1] = s.y1[q]; b[2] = s.x2[q]; b[3] = s.y2[q];
        cscores[row0 + q] = s.sc[q];
        csrc[row0 + q] = s.ind[q];
        ccls[row0 + q] = c;
        keep_idx[row0 + q] = q;
    }
    if (tid == 0) keep_cnt[p] = kept;
}

struct MroiSoftPlan { size_t boxes, scores, src, cls, keep, keepcnt, status, flat, total; };
static MroiSoftPlan mroi_soft_plan(int P, int nmax)
{
    MroiSoftPlan m; size_t o = 0;
    m.boxes = o; o += al256((size_t)P * nmax * 16);
    m.scores = o; o += al256((size_t)P * nmax * 4);
    m.src = o; o += al256((size_t)P * nmax * 4);
    m.cls = o; o += al256((size_t)P * nmax * 4);
    m.keep = o; o += al256((size_t)P * nmax * 4);
    m.keepcnt = o; o += al256((size_t)P * 4);
    m.status = o; o += 256;
    m.flat = o; o += al256((size_t)P * nmax * 4);
    m.total = o + 256;
    return m;
}

extern "C" size_t upsnet_mask_roi_soft_workspace_bytes(int N, int C)
{
    if (N < 1 || C < 2 || N > 8192) return 256;
    int P, nmax;
    mroi_dims(N, C, 0, &P, &nmax);
    return mroi_soft_plan(P, nmax).total;
}

extern "C" int upsnet_mask_roi_soft(void *stream, const float *rois, const float *bbox_delta, const float *cls_prob, int num_rois,
                                    const int *num_rois_dev, int num_classes, const float *im_info, int clip_boxes, float score_thresh,
                                    float nms_thresh, int max_det, const float reg_weights[4], int method, float sigma, float floor_thresh,
                                    float *boxes_out, float *scores_out, int64_t *cls_out, int *src_out, int *num_out, void *workspace)
{
    UPS_REQUIRE(rois && bbox_delta && cls_prob && im_info && reg_weights && boxes_out && scores_out && cls_out && src_out &&
                    num_out && workspace, "mask_roi_soft: null pointer");
    UPS_REQUIRE(num_rois >= 1 && num_classes >= 2, "mask_roi_soft: need at least one roi and two classes");
    UPS_REQUIRE(num_rois <= 8192, "mask_roi_soft: %d rois exceed the 8192 supported", num_rois);
    UPS_REQUIRE(method >= 0 && method <= 2, "mask_roi_soft: method must be 0 (hard), 1 (linear) or 2 (gaussian), got %d", method);
    UPS_REQUIRE(method != 2 || sigma > 0.f, "mask_roi_soft: the gaussian method needs sigma > 0 (got %g)", (double)sigma);   // (NaN fails too)
    UPS_REQUIRE(nms_thresh == nms_thresh && floor_thresh == floor_thresh, "mask_roi_soft: nms_thresh / floor is NaN");
    int P, nmax;
    mroi_dims(num_rois, num_classes, 0, &P, &nmax);
    const MroiSoftPlan m = mroi_soft_plan(P, nmax);
    unsigned char *ws = (unsigned char *)workspace;
    float *cboxes = (float *)(ws + m.boxes), *cscores = (float *)(ws + m.scores);
    int *csrc = (int *)(ws + m.src), *ccls = (int *)(ws + m.cls);
    int *keep = (int *)(ws + m.keep), *keepcnt = (int *)(ws + m.keepcnt), *status = (int *)(ws + m.status);
    hipStream_t st = (hipStream_t)stream;
    if (ups_zero_async(status, sizeof(int), st)) return 1;
    // threads and LDS from the most candidates a class can hold: one wavefront up to 1024 rows, four above (T * SNMS_KMAX positions)
    const int rows = nmax < SNMS_LDS_MAX ? nmax : SNMS_LDS_MAX;
    const int cap = (rows + 3) & ~3;
    const size_t smem = snms_lds_bytes(cap);
#define MROI_SOFT_ARGS rois, bbox_delta, cls_prob, num_rois, num_rois_dev, num_classes, im_info, clip_boxes, score_thresh, reg_weights[0], \
        reg_weights[1], reg_weights[2], reg_weights[3], nmax, cap, sigma, nms_thresh, floor_thresh, method, cboxes, cscores, csrc, ccls, keep, \
        keepcnt, status
    if (rows <= 64 * SNMS_KMAX) {
        hipLaunchKernelGGL(mroi_soft_kernel<64>, dim3(P), dim3(64), smem, st, MROI_SOFT_ARGS);
    } else {
        static std::atomic<unsigned long long> attr_dev{0};
        UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&mroi_soft_kernel<256>),
                                                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                        (int)snms_lds_bytes(SNMS_LDS_MAX))));
        hipLaunchKernelGGL(mroi_soft_kernel<256>, dim3(P), dim3(256), smem, st, MROI_SOFT_ARGS);
    }
#undef MROI_SOFT_ARGS
    UPS_CHECK_LAUNCH("mroi_soft_kernel");
    hipLaunchKernelGGL(mroi_finalize_kernel, dim3(1), dim3(DET_T), (size_t)(P + 1) * sizeof(int), st, P, nmax, max_det, cboxes, cscores, csrc, ccls, keep,
                       keepcnt, boxes_out, scores_out, cls_out, src_out, num_out, status, (unsigned *)(ws + m.flat));
    UPS_CHECK_LAUNCH("mroi_finalize_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// The reference runs the mask head twice (resnet_upsnet.py:190,215): on the per-class detections and on the class-agnostic
// "panoptic" detections. Both sets are selections from the same (ROI row, class) -> decoded-box table, so a panoptic
// detection that is also a per-class detection would get bit-identical mask logits (every ROI goes through the mask head
// independently). This kernel finds those duplicates by (source ROI, class): map[p] = row of panoptic detection p in the
// concatenation [set A ; unmatched of set B], and the unmatched boxes of B are compacted in order.
__global__ void __launch_bounds__(DET_T)
mroi_dedup_kernel(const int *__restrict__ a_src, const int64_t *__restrict__ a_cls, const int *__restrict__ na_dev, const int cap_a,
                  const int *__restrict__ b_src, const int64_t *__restrict__ b_cls, const float *__restrict__ b_boxes,
                  const int *__restrict__ nb_dev, const int cap_b, int *__restrict__ map_out, float *__restrict__ extra_boxes,
                  int *__restrict__ n_extra)
{
    __shared__ int sh[DET_T / 64 + 1];
    const int tid = threadIdx.x;
    const int na = min(*na_dev, cap_a), nb = min(*nb_dev, cap_b);
    int cnt = 0;
    for (int base = 0; base < nb; base += DET_T) {
        const int p = base + tid;
        int hit = -1;
        if (p < nb) {
            const int s = b_src[p];
            const int64_t c = b_cls[p];
            for (int j = 0; j < na; ++j)
                if (a_src[j] == s && a_cls[j] == c) { hit = j; break; }
        }
        const bool extra = p < nb && hit < 0;
        int tot;
        const int pos = cnt + det_block_scan(extra, sh, &tot);
        if (p < nb) map_out[p] = extra ? na + pos : hit;
        if (extra) {
#pragma unroll
            for (int q = 0; q < 5; ++q) extra_boxes[(long)pos * 5 + q] = b_boxes[(long)p * 5 + q];
        }
        cnt += tot;
    }
    for (int p = nb + tid; p < cap_b && p < MROI_FILL; p += DET_T) map_out[p] = 0;   // defined rows past the count
    if (tid == 0) *n_extra = cnt;
}

extern "C" int upsnet_mask_roi_dedup(void *stream, const int *a_src, const int64_t *a_cls, const int *num_a, int cap_a, const int *b_src,
                                     const int64_t *b_cls, const float *b_boxes, const int *num_b, int cap_b, int *map_out,
                                     float *extra_boxes, int *num_extra)
{
    UPS_REQUIRE(a_src && a_cls && num_a && b_src && b_cls && b_boxes && num_b && map_out && extra_boxes && num_extra,
                "mask_roi_dedup: null pointer");
    UPS_REQUIRE(cap_a >= 0 && cap_b >= 0, "mask_roi_dedup: bad capacity");
    hipLaunchKernelGGL(mroi_dedup_kernel, dim3(1), dim3(DET_T), 0, (hipStream_t)stream, a_src, a_cls, num_a, cap_a, b_src, b_cls, b_boxes,
                       num_b, cap_b, map_out, extra_boxes, num_extra);
    UPS_CHECK_LAUNCH("mroi_dedup_kernel");
    return 0;
}


// ---------------------------------------------------------------------------------------------
// pan_logit[k] = mask_logit[row[k]][cls[k]] (resnet_upsnet.py:215-221: the mask head's class plane of every panoptic detection), as
// ONE gather: out [K, hw] contiguous; the source is addressed by strides (NHWC or NCHW). Rows / classes are clamped so that the
// call can sit inside a captured graph on fixed-capacity buffers before the host knows the counts (rows past the count are ignored
// downstream). Replaces clamp + long + index_select (a [K, C, 28, 28] copy) + clamp + expand + gather = 6 launches.
__global__ void __launch_bounds__(256)
mask_logit_gather_kernel(const float *__restrict__ src, const int n_rows, const int C, const int hw, const long s_n, const long s_c,
                         const long s_e, const int *__restrict__ row, const int64_t *__restrict__ cls, float *__restrict__ out)
{
    const int k = blockIdx.x;
    const int r = min(max(row[k], 0), n_rows - 1);
    const int c = (int)min(max(cls[k], (int64_t)0), (int64_t)(C - 1));
    const float *__restrict__ sp = src + (long)r * s_n + (long)c * s_c;
    for (int e = threadIdx.x; e < hw; e += blockDim.x) out[(long)k * hw + e] = sp[(long)e * s_e];
}

extern "C" int upsnet_mask_logit_gather(void *stream, const float *mask_logit, int n_rows, int num_classes, int hw, long stride_n,
                                        long stride_c, long stride_e, const int *row, const int64_t *cls, int K, float *out)
{
    UPS_REQUIRE(mask_logit && row && cls && out, "mask_logit_gather: null pointer");
    UPS_REQUIRE(n_rows > 0 && num_classes > 0 && hw > 0 && K >= 0, "mask_logit_gather: bad sizes");
    if (K == 0) return 0;
    hipLaunchKernelGGL(mask_logit_gather_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, mask_logit, n_rows, num_classes, hw, stride_n,
                       stride_c, stride_e, row, cls, out);
    UPS_CHECK_LAUNCH("mask_logit_gather_kernel");
    return 0;
}
