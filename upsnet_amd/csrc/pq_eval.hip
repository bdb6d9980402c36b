// pq_eval.hip -- panoptic quality (PQ) and semantic confusion-matrix accumulation on the device: the scoring that follows
// get_unified_pan_result in the reference's test loop (BaseDataset.evaluate_panoptic -> _pq_compute_single_core,
// upsnet/dataset/base_dataset.py:209-330,514-610; BaseDataset.get_confusion_matrix, :806-824).
//
// Reference (numpy, host, one image per CPU worker): the prediction is recoloured to a panoptic PNG (_converter_2ch_single_core),
// np.unique over a uint64 (gt id, pred id) key per pixel gives every intersection, then the matching / FN / crowd / FP rules run
// over dicts. Here, integers only, three launches per image and a workspace sized once from max_gt:
//   pq_prep_kernel   one workgroup: the image's GT segments (JSON order) sorted by id (rank counting), and per category the row
//                    of its LAST crowd segment in JSON order (the reference's crowd_labels_dict is overwritten)
//   pq_hist_kernel   the pixel pass of pan_pixels.h over (pred key, gt id): runs counted into an LDS hash table per workgroup,
//                    one global atomic per distinct cell and workgroup (a full hash falls back to a global atomic);
//                    cells: pred area [key], inter(VOID, pred) [key], inter(gt row, pred) [row][inst] for equal categories only
//                    (the first arrival at a pred area cell appends the key to a list of the image's pred segments)
//   pq_match_kernel  one workgroup: matching (iou > 0.5 in float64), FP with VOID + crowd absorption over the listed pred segments,
//                    FN, and the additions into the running per-category accumulators; clears the cells it used, so the workspace
//                    is zero again afterwards
// A pred segment is a (cat, inst) pair with cat != 255, key = cat << 8 | inst < 65280; only same-category pairs can match or be
// absorbed by a crowd region, and a category holds at most 256 pred instances, so the joint table is [max_gt][256] whatever the
// number of distinct pred keys. The ids of the reference's pred PNG are colours, which relabel segments without changing any count.
#include "common.h"
#include "upsnet_hip.h"
#include "pq_eval.h"

__global__ void __launch_bounds__(256)
pq_hist_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ gt, const long npix, const bool vec, const int n,
               PqWs ws)
{
    extern __shared__ unsigned s_hist[];
    unsigned *s_key = s_hist;
    int *s_val = (int *)(s_hist + PQ_HASH);
    int *s_id = (int *)(s_hist + 2 * PQ_HASH);
    unsigned char *s_cat = (unsigned char *)(s_id + n);
    const int t = threadIdx.x;
    pan_lds_clear<PQ_HASH_BITS>(s_key, s_val, 1);
    for (int i = t; i < n; i += blockDim.x) { s_id[i] = ws.seg[i].id; s_cat[i] = (unsigned char)ws.seg[i].cat; }
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + t) * PAN_RUN;
    if (p0 < npix)
        pan_pair_walk<false>(pred, gt, nullptr, p0, npix, vec, [&](const unsigned pk, const int gid, unsigned, const int run) {
            pq_flush(s_key, s_val, ws, s_id, s_cat, n, pk, gid, run);
        });
    __syncthreads();
    pan_lds_drain<PQ_HASH_BITS>(s_key, [&](const unsigned k, const int i) { pq_global_add(ws, k, s_val[i]); });
}

__global__ void __launch_bounds__(PQM_T)
pq_match_kernel(const int n, const unsigned char *__restrict__ cat_known, const int image_index, PqWs ws, int64_t *__restrict__ tp,
                int64_t *__restrict__ fp, int64_t *__restrict__ fn, double *__restrict__ iou, unsigned long long *__restrict__ status)
{
    extern __shared__ int s_row[];   // [n]: cat | crowd << 8 | min(matches, 2) << 9
    __shared__ unsigned s_matched[PQ_KEYS / 32];
    __shared__ int s_known[256], s_fp[256];
    __shared__ int s_bad;
    const int t = threadIdx.x, lane = t & (UPS_WAVE - 1), wave = t / UPS_WAVE;
    int *__restrict__ cnt = ws.cnt;
    const int *__restrict__ joint = cnt + PQ_JOINT_OFF;
    for (int i = t; i < PQ_KEYS / 32; i += PQM_T) s_matched[i] = 0;
    for (int c = t; c < 256; c += PQM_T) { s_known[c] = cat_known[c]; s_fp[c] = 0; }
    if (t == 0) s_bad = 256;
    __syncthreads();
    // matching: one wave per GT row, lane l holds instances l, l+64, l+128, l+192
    for (int g = wave; g < n; g += PQM_WAVES) {
        const PqSeg s = ws.seg[g];
        int total = 0, mine = 0;
        double my_iou = 0.0;
        if (!s.crowd) {
            for (int j = 0; j < 4; ++j) {
                const int inst = lane + UPS_WAVE * j;
                const int inter = joint[g * 256 + inst];
                bool hit = false;
                if (inter > 0) {
                    const double v = pq_iou(cnt, s.area, s.cat, inst, inter);
                    if (v > 0.5) {
                        hit = true;
                        ++mine;
                        my_iou = v;
                        const int k = s.cat << 8 | inst;
                        atomicOr(&s_matched[k >> 5], 1u << (k & 31));
                    }
                }
                total += __popcll(__ballot(hit));
            }
        }
        if (total == 1 && mine == 1) ws.row_iou[g] = my_iou;
        if (lane == 0) s_row[g] = s.cat | s.crowd << 8 | min(total, 2) << 9;
    }
    __syncthreads();
    // unmatched pred segments: FP unless more than half of it lies on GT VOID + the category's crowd region; unknown categories
    const int nk = min(*ws.nkeys, PQ_KEYS);
    for (int i = t; i < nk; i += PQM_T) {
        const int k = ws.keys[i], a = cnt[k];
        const int cat = k >> 8;
        if (!s_known[cat]) atomicMin(&s_bad, cat);
        if (s_matched[k >> 5] >> (k & 31) & 1) continue;
        int inter = cnt[PQ_VOID_OFF + k];
        const int cr = ws.crowd_row[cat];
        if (cr >= 0) inter += joint[cr * 256 + (k & 255)];
        if (!((double)inter / (double)a > 0.5)) atomicAdd(&s_fp[cat], 1);
    }
    __syncthreads();
    if (s_bad != 256) {
        // the reference raises KeyError before adding anything for this image; the first error is kept for the host
        if (t == 0) atomicCAS(status, 0ull, (unsigned long long)(image_index + 1) << 8 | (unsigned)s_bad);
    } else if (t < 256) {
        // per category, matches added in ascending GT id (the reference's np.unique order) straight into the running sum
        const int c = t;
        double acc = iou[c];
        long long tpc = 0, fnc = 0;
        for (int g = 0; g < n; ++g) {
            const int r = s_row[g];
            if ((r & 511) != c) continue;   // other category, or crowd
            const int m = r >> 9;
            if (m == 0) {
                ++fnc;
            } else if (m == 1) {
                acc += ws.row_iou[g];
                ++tpc;
            } else {   // several matches of one GT segment (only with JSON areas below the pixel counts): instance order
                const long long area_g = ws.seg[g].area;
                for (int inst = 0; inst < 256; ++inst) {
                    const int inter = joint[g * 256 + inst];
                    if (inter > 0) {
                        const double v = pq_iou(cnt, area_g, c, inst, inter);
                        if (v > 0.5) { acc += v; ++tpc; }
                    }
                }
            }
        }
        iou[c] = acc;
        tp[c] += tpc;
        fn[c] += fnc;
        fp[c] += s_fp[c];
    }
    __syncthreads();
    // leave the workspace zeroed for the next image
    for (int i = t; i < nk; i += PQM_T) {
        const int k = ws.keys[i];
        cnt[k] = 0;
        cnt[PQ_VOID_OFF + k] = 0;   // VOID cells are only ever counted for keys with an area
    }
    for (int i = t; i < n * 256; i += PQM_T) cnt[PQ_JOINT_OFF + i] = 0;
    if (t == 0) *ws.nkeys = 0;
}

extern "C" size_t upsnet_pq_workspace_bytes(int max_gt)
{
    if (max_gt < 0 || max_gt > PQ_MAX_GT) return 0;
    return pq_cnt_cells(max_gt) * sizeof(int) + (size_t)max_gt * (sizeof(PqSeg) + sizeof(double)) + (256 + 2 + PQ_KEYS) * sizeof(int);
}

extern "C" int upsnet_pq_accumulate(void *stream, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                                    const int64_t *segments, int num_segments, const unsigned char *cat_known, int image_index, int max_gt,
                                    void *workspace, int64_t *tp, int64_t *fp, int64_t *fn, double *iou, uint64_t *status)
{
    UPS_REQUIRE(pred_2ch && gt_rgb && cat_known && workspace && tp && fp && fn && iou && status && (segments || num_segments == 0),
                "pq_accumulate: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "pq_accumulate: bad image size %d x %d", height, width);
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PQ_MAX_GT, "pq_accumulate: max_gt %d outside 0..%d", max_gt, PQ_MAX_GT);
    UPS_REQUIRE(num_segments >= 0 && num_segments <= max_gt, "pq_accumulate: %d GT segments, workspace sized for %d", num_segments, max_gt);
    UPS_REQUIRE(image_index >= 0 && image_index < (1 << 24), "pq_accumulate: image index %d outside 0..2^24-1", image_index);
    UPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "pq_accumulate: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const PqWs ws = pq_ws(workspace, pq_cnt_cells(max_gt), max_gt);
    const int n = num_segments;
    const long npix = (long)height * width;
    hipLaunchKernelGGL(pq_prep_kernel, dim3(1), dim3(1024), (size_t)n * 2 * sizeof(int), st, segments, n, ws);   // n == 0: crowd rows reset
    UPS_CHECK_LAUNCH("pq_prep_kernel");
    const bool vec = (((uintptr_t)pred_2ch | (uintptr_t)gt_rgb) & 15) == 0;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const size_t lds = (size_t)PQ_HASH * 2 * sizeof(int) + (size_t)n * (sizeof(int) + 1);
    hipLaunchKernelGGL(pq_hist_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), lds, st, pred_2ch, gt_rgb, npix, vec, n, ws);
    UPS_CHECK_LAUNCH("pq_hist_kernel");
    hipLaunchKernelGGL(pq_match_kernel, dim3(1), dim3(PQM_T), (size_t)n * sizeof(int), st, n, cat_known, image_index, ws, tp, fp, fn, iou,
                       (unsigned long long *)status);
    UPS_CHECK_LAUNCH("pq_match_kernel");
    return 0;
}


// ---------------------------------------------------------------------------------------------
// get_confusion_matrix (base_dataset.py:806-824): index = gt * C + pred (int32), np.bincount, cells index < C*C kept -- so a pred
// value >= C lands in another cell of the matrix (gt * C + pred = (gt + pred / C) * C + pred % C), exactly like the reference.
// Pixels with gt == ignore_label are dropped first (evaluate_ssegs, cityscapes.py:460-462); ignore_label < 0 drops nothing.
// One pass, 16 pixels per thread run-length compressed, an LDS-privatised C*C table when it fits (else global atomics).
#define CM_LDS_MAX_CELLS 8192

__global__ void __launch_bounds__(256)
confusion_kernel(const unsigned char *__restrict__ gt, const unsigned char *__restrict__ pred, const long npix, const int C, const int ignore,
                 const bool vec, const bool use_lds, unsigned long long *__restrict__ out)
{
    extern __shared__ int s_cm[];
    const int cells = C * C, t = threadIdx.x;
    if (use_lds) {
        for (int i = t; i < cells; i += blockDim.x) s_cm[i] = 0;
        __syncthreads();
    }
    const long p0 = ((long)blockIdx.x * blockDim.x + t) * PAN_RUN;
    if (p0 < npix) {
        unsigned gw[4], pw[4];
        if (vec && p0 + PAN_RUN <= npix) {
            const uint4 a = *(const uint4 *)(gt + p0), b = *(const uint4 *)(pred + p0);
            gw[0] = a.x; gw[1] = a.y; gw[2] = a.z; gw[3] = a.w;
            pw[0] = b.x; pw[1] = b.y; pw[2] = b.z; pw[3] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) gw[j] = pw[j] = 0;
#pragma unroll
            for (int j = 0; j < PAN_RUN; ++j)
                if (p0 + j < npix) {
                    gw[j >> 2] |= (unsigned)gt[p0 + j] << (8 * (j & 3));
                    pw[j >> 2] |= (unsigned)pred[p0 + j] << (8 * (j & 3));
                }
        }
        int key = -1, run = 0;
#define CM_FLUSH()                                                          \
    if (run && key >= 0 && key < cells) {                                   \
        if (use_lds) atomicAdd(&s_cm[key], run);                            \
        else atomicAdd(&out[key], (unsigned long long)run);                 \
    }
#pragma unroll
        for (int i = 0; i < PAN_RUN; ++i) {
            if (p0 + i < npix) {
                const int g = (int)pan_byte(gw, i), p = (int)pan_byte(pw, i);
                const int k = g == ignore ? -1 : g * C + p;
                if (k != key) { CM_FLUSH() key = k; run = 0; }
                ++run;
            }
        }
        CM_FLUSH()
#undef CM_FLUSH
    }
    if (use_lds) {
        __syncthreads();
        for (int i = t; i < cells; i += blockDim.x) {
            const int v = s_cm[i];
            if (v) atomicAdd(&out[i], (unsigned long long)v);
        }
    }
}

extern "C" int upsnet_confusion_accumulate(void *stream, const unsigned char *gt_label, const unsigned char *pred_label, long npix,
                                           int class_num, int ignore_label, int64_t *confusion)
{
    UPS_REQUIRE(gt_label && pred_label && confusion, "confusion_accumulate: null pointer");
    UPS_REQUIRE(npix >= 0 && npix < (1L << 40), "confusion_accumulate: bad pixel count %ld", npix);
    UPS_REQUIRE(class_num >= 1 && class_num <= 256, "confusion_accumulate: class_num %d outside 1..256", class_num);
    UPS_REQUIRE(ignore_label >= -1 && ignore_label <= 255, "confusion_accumulate: ignore_label %d outside -1..255", ignore_label);
    if (npix == 0) return 0;
    const int cells = class_num * class_num;
    const bool use_lds = cells <= CM_LDS_MAX_CELLS;
    const bool vec = (((uintptr_t)gt_label | (uintptr_t)pred_label) & 15) == 0;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), use_lds ? (size_t)cells * sizeof(int) : 0,
                       (hipStream_t)stream, gt_label, pred_label, npix, class_num, ignore_label, vec, use_lds,
                       (unsigned long long *)confusion);
    UPS_CHECK_LAUNCH("confusion_kernel");
    return 0;
}
