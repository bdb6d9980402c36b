// video_eval.hip -- Video Panoptic Quality (VPQ; Kim et al., CVPR 2020) and Segmentation and Tracking Quality (STQ; Weber et al.,
// NeurIPS 2021) of tracked sequences, counted on the device (the rules are stated in include/upsnet_hip.h and restated
// in plain numpy in tests/video_pq_ref.py). The reference has no video metric.
//
// Everything both metrics need is an integer count of one of four kinds of CELL, a 30-bit word kind << 28 | index:
//   JOINT  row << 16 | key   pixels of GT row `row` under pred key `key` (c << 8 | j, c != 255), WHATEVER their categories
//   AREA_P key               pixels of the pred key
//   VOID   key               pixels of the pred key on ignored GT (id 0, or an id that is not in the sequence table)
//   AREA_G row               pixels of the GT row (under any prediction, VOID included)
// VPQ reads the same-category JOINT cells, STQ's association the thing x thing ones, the confusion matrix is the JOINT cells summed by
// (cat(row), cat(key)) plus AREA_G - sum for pred VOID, and the pred pixels on thing-crowd GT are the JOINT cells of those rows.
// A dense joint table would be 4096 x 65536 ints, so all cells live in the global cell tables of pan_pixels.h (open addressing, the
// claimer of a slot appends it to a list, so nothing ever scans a table).
// Per frame, three launches:
//   ve_hist_kernel     ONE pass over the pixels, whatever `windows` is: the pixel pass of pan_pixels.h (pair walk, LDS hash per
//                      workgroup, one global atomic per distinct cell and workgroup)
//   ve_compact_kernel  the frame's touched slots -> the frame's (cell, count) list in a ring of the last max_window frames, and added
//                      into the sequence-level table; the frame table is left zero; unknown pred categories are reported
//   ve_window_kernel   one workgroup per window length n whose window ends at this frame: the n lists are sorted by cell in LDS
//                      (sort.h), equal cells summed, every other count found by binary search; TP by iou > 0.5 in float64, FP with
//                      VOID + all crowd rows of the category, FN; per category the matches are added in ascending row (= GT id)
//                      order straight into the running float64 sum, so the sum's order is: sequences, window starts, ids
// and per sequence two more (ve_seq_kernel, ve_reset_kernel): the sequence-level cells are delivered as one (cell, count) list that
// travels to the host by one asynchronous copy -- STQ's few float64 operations run there, from integers -- and every part of the
// workspace is zero again. Nothing between the first frame and the end of a sequence waits for the host.
// A table that is full (PAN_TABLE_PROBES slots in a row taken) or a window of more than VE_SORT list entries never loses a count silently: a
// bit of status[0] is set and the host raises RuntimeError at its next synchronisation.
#include "common.h"
#include "upsnet_hip.h"
#include "pq_eval.h"
#include "sort.h"

#define VE_JOINT 0u
#define VE_AREA_P 1u
#define VE_VOID 2u
#define VE_AREA_G 3u
#define VE_KIND(k) ((unsigned)(k) << 28)
#define VE_SEQ_BITS 15                    // sequence-level table: 32768 slots
#define VE_SEQ_SLOTS (1 << VE_SEQ_BITS)
#define VE_SORT 8192                      // list entries one window pass can merge (64 KiB of LDS keys)
#define VE_MAX_WINDOW 8
#define VE_T 1024
#define VE_FULL_FRAME 1ull
#define VE_FULL_SEQ 2ull
#define VE_FULL_WINDOW 4ull
#define VE_ROW_PRESENT (1 << 9)
#define VE_ROW_MATCHED (1 << 10)

// Workspace (all of it zero between sequences): int hdr[16] ([0] frame list length, [1] sequence list length) | ring_n[8] | ring_hi[8]
// | frame table uint[2 * HC] | frame slots int[HC] | sequence table uint[2 * SS] | sequence slots int[SS] | ring uint[K][2 * HC]
struct VeWs {
    int *hdr, *ring_n, *ring_hi;
    unsigned *ftab;
    int *fslots;
    unsigned *stab;
    int *sslots;
    unsigned *ring;
    int fbits;      // log2 of the frame table's slots
};

static inline size_t ve_ws_ints(int bits, int K) { return 32 + 3 * ((size_t)1 << bits) + 3 * (size_t)VE_SEQ_SLOTS + (size_t)K * 2 * ((size_t)1 << bits); }

static inline VeWs ve_ws(void *base, int max_gt, long npix, int K)
{
    VeWs w;
    w.fbits = pan_frame_bits(npix);
    const size_t HC = (size_t)1 << w.fbits;
    int *p = (int *)base;
    w.hdr = p;
    w.ring_n = p + 16;
    w.ring_hi = p + 24;
    p += 32;
    w.ftab = (unsigned *)p;
    p += 2 * HC;
    w.fslots = p;
    p += HC;
    w.stab = (unsigned *)p;
    p += 2 * VE_SEQ_SLOTS;
    w.sslots = p;
    p += VE_SEQ_SLOTS;
    w.ring = (unsigned *)p;
    return w;
}

// count v > 0 of one cell of the frame: the workgroup's LDS table, or the frame table when that is full around the cell's slot
__device__ static inline void ve_lds_add(unsigned *s_key, int *s_val, const VeWs &ws, unsigned long long *status, const unsigned cell, const int v)
{
    if (!pan_lds_count<PQ_HASH_BITS>(s_key, s_val, cell, v))
        pan_table_add(ws.ftab, ws.fbits, ws.fslots, &ws.hdr[0], status, VE_FULL_FRAME, cell, (unsigned)v);
}

// one run of `run` pixels with the same pred key and GT id
__device__ static inline void ve_flush(unsigned *s_key, int *s_val, const VeWs &ws, unsigned long long *status, const int *s_id, const int n,
                                       const unsigned pk, const int gid, const int run)
{
    const int g = gid == 0 ? -1 : pq_find(s_id, n, gid);      // ids not in the sequence table are ignored, like 0
    const bool pred = (pk >> 8) != 255;                       // pred VOID, whatever its instance, is no key
    if (pred) {
        ve_lds_add(s_key, s_val, ws, status, VE_KIND(VE_AREA_P) | pk, run);
        if (g < 0) ve_lds_add(s_key, s_val, ws, status, VE_KIND(VE_VOID) | pk, run);
    }
    if (g >= 0) {
        ve_lds_add(s_key, s_val, ws, status, VE_KIND(VE_AREA_G) | (unsigned)g, run);
        if (pred) ve_lds_add(s_key, s_val, ws, status, VE_KIND(VE_JOINT) | (unsigned)g << 16 | pk, run);
    }
}

// table: int[2 * n] rows in ascending id (id, cat | crowd << 8), then int[ncrowd] the crowd rows
__global__ void __launch_bounds__(256)
ve_hist_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ gt, const long npix, const bool vec,
               const int *__restrict__ table, const int n, VeWs ws, unsigned long long *__restrict__ status)
{
    extern __shared__ unsigned s_hist[];
    unsigned *s_key = s_hist;
    int *s_val = (int *)(s_hist + PQ_HASH);
    int *s_id = (int *)(s_hist + 2 * PQ_HASH);
    const int t = threadIdx.x;
    pan_lds_clear<PQ_HASH_BITS>(s_key, s_val, 1);
    for (int i = t; i < n; i += blockDim.x) s_id[i] = table[2 * i];
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + t) * PAN_RUN;
    if (p0 < npix)
        pan_pair_walk<false>(pred, gt, nullptr, p0, npix, vec, [&](const unsigned pk, const int gid, unsigned, const int run) {
            ve_flush(s_key, s_val, ws, status, s_id, n, pk, gid, run);
        });
    __syncthreads();
    pan_lds_drain<PQ_HASH_BITS>(s_key, [&](const unsigned k, const int i) {
        pan_table_add(ws.ftab, ws.fbits, ws.fslots, &ws.hdr[0], status, VE_FULL_FRAME, k, (unsigned)s_val[i]);
    });
}

// the frame's touched slots -> ring list `slotk` and the sequence table; the frame table and its slot list are zero afterwards
// (hdr[0], the list's length, is cleared by the window pass that follows: every workgroup here reads it)
__global__ void __launch_bounds__(256)
ve_compact_kernel(VeWs ws, const int slotk, const unsigned char *__restrict__ cat_known, const long long where,
                  unsigned long long *__restrict__ status)
{
    const int cap = 1 << ws.fbits;
    const int n = min(max(ws.hdr[0], 0), cap);
    unsigned *__restrict__ list = ws.ring + (size_t)slotk * 2 * cap;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int slot = ws.fslots[i] & (cap - 1);
        const unsigned k = ws.ftab[2 * slot], v = ws.ftab[2 * slot + 1];
        ws.ftab[2 * slot] = 0;
        ws.ftab[2 * slot + 1] = 0;
        ws.fslots[i] = 0;
        list[2 * i] = k;
        list[2 * i + 1] = v;
        if (k == 0) continue;   // (only a slot list that was not zero to begin with)
        const unsigned cell = k - 1;
        if (cell >> 28 == VE_AREA_P && !cat_known[(cell >> 8) & 255])
            atomicMin(status + 1, (unsigned long long)(where | (long long)((cell >> 8) & 255)));   // the first frame, its lowest category
        pan_table_add(ws.stab, VE_SEQ_BITS, ws.sslots, &ws.hdr[1], status, VE_FULL_SEQ, cell, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ws.ring_n[slotk] = n;
        ws.ring_hi[slotk] = max(ws.ring_hi[slotk], n);   // what the end of the sequence has to clear
    }
}

struct VeWin {
    int n[VE_MAX_WINDOW];
};

__device__ static inline unsigned ve_cell_at(const ups_u64 *s_keys, const int i) { return 0x40000000u - (unsigned)(s_keys[i] >> 32); }

// the summed count of a cell of the sorted window list (0 if it has none): the first entry of a cell holds its sum
__device__ static inline unsigned ve_lookup(const ups_u64 *s_keys, const int total, const unsigned cell)
{
    int lo = 0, hi = total;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ve_cell_at(s_keys, mid) < cell) lo = mid + 1;
        else hi = mid;
    }
    return lo < total && ve_cell_at(s_keys, lo) == cell ? (unsigned)s_keys[lo] : 0u;
}

// workgroup w scores the window of win.n[w] frames that ends at frame `frame` of the sequence (none if the sequence is still shorter)
__global__ void __launch_bounds__(VE_T)
ve_window_kernel(VeWs ws, const int *__restrict__ table, const int nrows, const int ncrowd, const VeWin win, const int K,
                 const int frame, int64_t *__restrict__ tp, int64_t *__restrict__ fp, int64_t *__restrict__ fn, double *__restrict__ iou,
                 unsigned long long *__restrict__ status)
{
    extern __shared__ __attribute__((aligned(16))) ups_u64 s_keys[];   // [VE_SORT] | double s_iou[nrows] | int s_fp[256] | unsigned s_matched[2048] | int s_row[nrows]
    double *s_iou = (double *)(s_keys + VE_SORT);              // the iou of a matched row (in LDS: the ordered sum below reads it row by row)
    int *s_fp = (int *)(s_iou + nrows);
    unsigned *s_matched = (unsigned *)(s_fp + 256);
    int *s_row = (int *)(s_matched + PQ_KEYS / 32);            // cat | crowd << 8 | present << 9 | matched << 10
    const int t = threadIdx.x, w = blockIdx.x, n = win.n[w];
    if (w == 0 && t == 0) ws.hdr[0] = 0;                       // the compaction before this launch was the last reader
    if (frame + 1 < n) return;
    const int cap = 1 << ws.fbits;
    int total = 0;
    for (int j = 0; j < n; ++j) total += min(max(ws.ring_n[(frame - j) % K], 0), cap);
    if (total > VE_SORT) {
        if (t == 0) atomicOr(status, VE_FULL_WINDOW);
        return;
    }
    const int M = ups_next_pow2(total);
    int off = 0;
    for (int j = 0; j < n; ++j) {
        const int slotk = (frame - j) % K, cnt = min(max(ws.ring_n[slotk], 0), cap);
        const unsigned *__restrict__ list = ws.ring + (size_t)slotk * 2 * cap;
        // ascending cells under a descending sort: the key's high word is 2^30 + 1 - (cell + 1), never 0
        for (int i = t; i < cnt; i += VE_T) s_keys[off + i] = (ups_u64)(0x40000001u - list[2 * i]) << 32 | list[2 * i + 1];
        off += cnt;
    }
    for (int i = total + t; i < M; i += VE_T) s_keys[i] = 0ull;
    for (int g = t; g < nrows; g += VE_T) s_row[g] = table[2 * g + 1] & 511;
    for (int i = t; i < PQ_KEYS / 32; i += VE_T) s_matched[i] = 0;
    if (t < 256) s_fp[t] = 0;
    ups_block_sort_desc(s_keys, M);
    // equal cells are neighbours now: the first entry of each takes the sum (n <= 8 frames of <= 2^24 pixels: 32 bits hold it)
    unsigned sums[VE_SORT / VE_T];
#pragma unroll
    for (int r = 0; r < VE_SORT / VE_T; ++r) {
        const int i = t + r * VE_T;
        sums[r] = 0;
        if (i < total) {
            const unsigned cell = ve_cell_at(s_keys, i);
            if (i == 0 || ve_cell_at(s_keys, i - 1) != cell) {
                unsigned s = 0;
                for (int j = i; j < total && ve_cell_at(s_keys, j) == cell; ++j) s += (unsigned)s_keys[j];
                sums[r] = s;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < VE_SORT / VE_T; ++r) {
        const int i = t + r * VE_T;
        if (i < total) s_keys[i] = (s_keys[i] & 0xffffffff00000000ull) | sums[r];   // (0 for the later entries of a cell: never read)
    }
    __syncthreads();
    // rows present in the window; TP: same category, non-crowd row, iou > 0.5 in float64 (at most one per row and per key)
    for (int i = t; i < total; i += VE_T) {
        const unsigned inter = (unsigned)s_keys[i];
        if (inter == 0) continue;
        const unsigned cell = ve_cell_at(s_keys, i), kind = cell >> 28;
        if (kind == VE_AREA_G) {
            const int row = cell & 0xfff;
            if (row < nrows) atomicOr(&s_row[row], VE_ROW_PRESENT);
        } else if (kind == VE_JOINT) {
            const int row = (cell >> 16) & 0xfff;
            const unsigned pk = cell & 0xffff;
            if (row >= nrows) continue;
            const int r = s_row[row] & 511;
            if (r != (int)(pk >> 8)) continue;    // other category, or a crowd row
            const long long uni = (long long)ve_lookup(s_keys, total, VE_KIND(VE_AREA_P) | pk) + (long long)ve_lookup(s_keys, total, VE_KIND(VE_AREA_G) | (unsigned)row)
                                  - (long long)inter - (long long)ve_lookup(s_keys, total, VE_KIND(VE_VOID) | pk);
            const double v = (double)inter / (double)uni;
            if (v > 0.5) {
                atomicOr(&s_row[row], VE_ROW_MATCHED);
                atomicOr(&s_matched[pk >> 5], 1u << (pk & 31));
                s_iou[row] = v;
            }
        }
    }
    __syncthreads();
    // FP: an unmatched key, unless more than half of it lies on ignored GT + ALL crowd rows of its category
    const int *__restrict__ crowd_rows = table + 2 * nrows;
    for (int i = t; i < total; i += VE_T) {
        const unsigned a = (unsigned)s_keys[i];
        const unsigned cell = ve_cell_at(s_keys, i);
        if (a == 0 || cell >> 28 != VE_AREA_P) continue;
        const unsigned pk = cell & 0xffff;
        if (s_matched[pk >> 5] >> (pk & 31) & 1) continue;
        long long ign = ve_lookup(s_keys, total, VE_KIND(VE_VOID) | pk);
        for (int q = 0; q < ncrowd; ++q) {
            const int g = crowd_rows[q];
            if (g >= 0 && g < nrows && (s_row[g] & 255) == (int)(pk >> 8)) ign += ve_lookup(s_keys, total, VE_KIND(VE_JOINT) | (unsigned)g << 16 | pk);
        }
        if (!((double)ign / (double)a > 0.5)) atomicAdd(&s_fp[pk >> 8], 1);
    }
    __syncthreads();
    if (t < 256) {
        // per category, the matches in ascending row (= GT id) order straight into the running sum
        const int c = t;
        double acc = iou[w * 256 + c];
        long long tpc = 0, fnc = 0;
        for (int g = 0; g < nrows; ++g) {
            const int r = s_row[g];
            if ((r & 511) != c || !(r & VE_ROW_PRESENT)) continue;   // other category, crowd, or no pixel in this window
            if (r & VE_ROW_MATCHED) {
                acc += s_iou[g];
                ++tpc;
            } else {
                ++fnc;
            }
        }
        iou[w * 256 + c] = acc;
        tp[w * 256 + c] += tpc;
        fn[w * 256 + c] += fnc;
        fp[w * 256 + c] += s_fp[c];
    }
}

// the sequence-level cells -> out[0] = their number, out[2 + 2 i], out[3 + 2 i] = (cell + 1, count); the sequence table, its slot list
// and the ring lists are zero afterwards (the header words by ve_reset_kernel: every workgroup here reads them)
__global__ void __launch_bounds__(256)
ve_seq_kernel(VeWs ws, const int K, unsigned *__restrict__ out)
{
    const int cap = 1 << ws.fbits;
    const int n = min(max(ws.hdr[1], 0), VE_SEQ_SLOTS);
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    for (int i = tid; i < n; i += step) {
        const int slot = ws.sslots[i] & (VE_SEQ_SLOTS - 1);
        out[2 + 2 * i] = ws.stab[2 * slot];
        out[3 + 2 * i] = ws.stab[2 * slot + 1];
        ws.stab[2 * slot] = 0;
        ws.stab[2 * slot + 1] = 0;
        ws.sslots[i] = 0;
    }
    if (tid == 0) { out[0] = (unsigned)n; out[1] = 0; }
    for (int k = 0; k < K; ++k) {
        const int hi = min(max(ws.ring_hi[k], 0), cap);
        unsigned *__restrict__ list = ws.ring + (size_t)k * 2 * cap;
        for (int i = tid; i < 2 * hi; i += step) list[i] = 0;
    }
}

__global__ void ve_reset_kernel(VeWs ws)
{
    if (threadIdx.x < 32) ws.hdr[threadIdx.x] = 0;   // hdr, ring_n, ring_hi
}

extern "C" size_t upsnet_video_eval_workspace_bytes(int max_gt, int height, int width, int max_window)
{
    if (max_gt < 0 || max_gt > PQ_MAX_GT || height <= 0 || width <= 0 || (long)height * width > (1L << 24) || max_window < 1 ||
        max_window > VE_MAX_WINDOW)
        return 0;
    return ve_ws_ints(pan_frame_bits((long)height * width), max_window) * sizeof(int);
}

extern "C" size_t upsnet_video_eval_sequence_ints(void) { return 2 + 2 * (size_t)VE_SEQ_SLOTS; }

extern "C" int upsnet_video_eval_frame(void *stream, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                                       const int *table, int num_rows, int num_crowd, int max_gt, const int *windows, int num_windows,
                                       int max_window, int frame, int sequence, const unsigned char *cat_known, void *workspace, int64_t *tp,
                                       int64_t *fp, int64_t *fn, double *iou, uint64_t *status)
{
    UPS_REQUIRE(pred_2ch && gt_rgb && windows && cat_known && workspace && tp && fp && fn && iou && status && (table || num_rows == 0),
                "video_eval_frame: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "video_eval_frame: bad frame size %d x %d", height, width);
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PQ_MAX_GT, "video_eval_frame: max_gt %d outside 0..%d", max_gt, PQ_MAX_GT);
    UPS_REQUIRE(num_rows >= 0 && num_rows <= max_gt, "video_eval_frame: %d GT rows, more than max_gt %d", num_rows, max_gt);
    UPS_REQUIRE(num_crowd >= 0 && num_crowd <= num_rows, "video_eval_frame: %d crowd rows of %d rows", num_crowd, num_rows);
    UPS_REQUIRE(max_window >= 1 && max_window <= VE_MAX_WINDOW, "video_eval_frame: max_window %d outside 1..%d", max_window, VE_MAX_WINDOW);
    UPS_REQUIRE(num_windows >= 1 && num_windows <= VE_MAX_WINDOW, "video_eval_frame: %d windows outside 1..%d", num_windows, VE_MAX_WINDOW);
    VeWin win;
    for (int i = 0; i < VE_MAX_WINDOW; ++i) win.n[i] = 0;
    for (int i = 0; i < num_windows; ++i) {
        UPS_REQUIRE(windows[i] >= 1 && windows[i] <= max_window && (i == 0 || windows[i] > windows[i - 1]),
                    "video_eval_frame: windows must be ascending, unique and in 1..max_window");
        win.n[i] = windows[i];
    }
    UPS_REQUIRE(frame >= 0 && frame < (1 << 24), "video_eval_frame: frame %d outside 0..2^24-1", frame);
    UPS_REQUIRE(sequence >= 0 && sequence < (1 << 30), "video_eval_frame: sequence %d outside 0..2^30-1", sequence);
    UPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "video_eval_frame: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)height * width;
    const VeWs ws = ve_ws(workspace, max_gt, npix, max_window);
    unsigned long long *stat = (unsigned long long *)status;
    const bool vec = (((uintptr_t)pred_2ch | (uintptr_t)gt_rgb) & 15) == 0;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    hipLaunchKernelGGL(ve_hist_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), (size_t)(2 * PQ_HASH + num_rows) * sizeof(int), st,
                       pred_2ch, gt_rgb, npix, vec, table, num_rows, ws, stat);
    UPS_CHECK_LAUNCH("ve_hist_kernel");
    const long long where = (long long)sequence << 32 | (long long)frame << 8;
    hipLaunchKernelGGL(ve_compact_kernel, dim3(min(64, 1 << (ws.fbits - 8))), dim3(256), 0, st, ws, frame % max_window, cat_known, where, stat);
    UPS_CHECK_LAUNCH("ve_compact_kernel");
    const size_t lds = (size_t)VE_SORT * sizeof(ups_u64) + (size_t)num_rows * sizeof(double) + (256 + PQ_KEYS / 32 + (size_t)num_rows) * sizeof(int);
    static std::atomic<unsigned long long> attr_dev{0};
    UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&ve_window_kernel),
                                                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                                                    (int)(VE_SORT * sizeof(ups_u64) + PQ_MAX_GT * sizeof(double) + (256 + PQ_KEYS / 32 + PQ_MAX_GT) * sizeof(int)))));
    hipLaunchKernelGGL(ve_window_kernel, dim3(num_windows), dim3(VE_T), lds, st, ws, table, num_rows, num_crowd, win, max_window, frame,
                       tp, fp, fn, iou, stat);
    UPS_CHECK_LAUNCH("ve_window_kernel");
    return 0;
}

extern "C" int upsnet_video_eval_end(void *stream, int height, int width, int max_gt, int max_window, void *workspace, int *sequence_out,
                                     int *host_out)
{
    UPS_REQUIRE(workspace && sequence_out, "video_eval_end: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "video_eval_end: bad frame size %d x %d", height, width);
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PQ_MAX_GT, "video_eval_end: max_gt %d outside 0..%d", max_gt, PQ_MAX_GT);
    UPS_REQUIRE(max_window >= 1 && max_window <= VE_MAX_WINDOW, "video_eval_end: max_window %d outside 1..%d", max_window, VE_MAX_WINDOW);
    hipStream_t st = (hipStream_t)stream;
    const VeWs ws = ve_ws(workspace, max_gt, (long)height * width, max_window);
    hipLaunchKernelGGL(ve_seq_kernel, dim3(256), dim3(256), 0, st, ws, max_window, (unsigned *)sequence_out);
    UPS_CHECK_LAUNCH("ve_seq_kernel");
    hipLaunchKernelGGL(ve_reset_kernel, dim3(1), dim3(64), 0, st, ws);
    UPS_CHECK_LAUNCH("ve_reset_kernel");
    if (host_out)
        UPS_CHECK_HIP(hipMemcpyAsync(host_out, sequence_out, (2 + 2 * (size_t)VE_SEQ_SLOTS) * sizeof(int), hipMemcpyDeviceToHost, st));
    return 0;
}
