// mots_eval.hip -- the MOTS measures (Voigtlaender et al., MOTS: Multi-Object Tracking and Segmentation, CVPR 2019: sMOTSA, MOTSA, MOTSP,
// IDS, Frag, MT / PT / ML) of tracked sequences, counted on the device (the rules are stated in include/upsnet_hip.h and
// restated in plain numpy in tests/mots_ref.py, never compared with a build of mots_tools). The reference has no video metric.
//
// Masks are disjoint on both sides, so a match at IoU > 0.5 is unique and the whole metric is integer counting plus four words of
// state per GT row. A frame's counts are CELLS kind << 28 | index of a global cell table of pan_pixels.h, as in video_eval.hip:
//   JOINT  row << 16 | key   pixels of the scored GT row (thing, non-crowd) under a pred key of the SAME category
//   AREA_P key               pixels of the pred key (every key whose category is not a known stuff category)
//   IGN    key               pixels of the key on its category's ignore region: GT id 0 or not in the table, or a crowd row of its category
//   AREA_G row               pixels of the scored GT row
// Per frame, three launches:
//   mots_hist_kernel   ONE pass over the pixels: the pixel pass of pan_pixels.h (pair walk, LDS hash per workgroup, one global atomic
//                      per distinct cell and workgroup)
//   mots_match_kernel  one thread per cell of the frame's list: a JOINT cell looks its two areas up and applies 3 I > A_g + A_p in
//                      int64 (the row's partner goes into the row scratch, the key's bit into the matched set); an AREA_P cell looks
//                      its IGN count up and joins the frame's key list with its exemption flag; unknown categories are reported
//   mots_state_kernel  workgroup 0: last / gap / present / tracked of every row, then one thread per category adds the frame's
//                      counts in ascending row (= GT id) order, soft[] straight into the running float64 sum; the other workgroups
//                      count the unmatched keys (FP, or exempt) and leave the frame table, both lists and the matched set zero
// and one per sequence (mots_end_kernel): MT / PT / ML of every row that was present, and every part of the workspace zero again.
// The two list lengths are double-buffered by the frame's parity: a frame's match pass clears the pair of the frame before, whose
// last reader ended with the launch before. A full table (PAN_TABLE_PROBES slots in a row taken) never loses a count silently: bit 1 of
// status[0] is set and the host raises RuntimeError at its next synchronisation.
#include "common.h"
#include "upsnet_hip.h"
#include "pq_eval.h"

#define MOTS_JOINT 0u
#define MOTS_AREA_P 1u
#define MOTS_IGN 2u
#define MOTS_AREA_G 3u
#define MOTS_KIND(k) ((unsigned)(k) << 28)
#define MOTS_T 1024
#define MOTS_FULL_FRAME 1ull
#define MOTS_KBITS (PQ_KEYS / 32)
#define MOTS_ROW_CROWD (1 << 8)
#define MOTS_ROW_THING (1 << 9)
#define MOTS_CAT_KNOWN 1
#define MOTS_CAT_THING 2
// s_flag of the state pass: category (511: not scored) | present << 9 | matched << 10 | switch << 11 | fragmentation << 12
#define MOTS_F_PRESENT (1 << 9)
#define MOTS_F_MATCHED (1 << 10)
#define MOTS_F_IDS (1 << 11)
#define MOTS_F_FRAG (1 << 12)
enum { MOTS_TP = 0, MOTS_FP, MOTS_FN, MOTS_GT, MOTS_IDS, MOTS_FRAG, MOTS_FP_IGN, MOTS_COUNTS };

// Workspace (all of it zero between sequences, everything but the row state zero between frames): int hdr[16] ([0], [1] frame list
// length by frame parity, [2], [3] key list length) | matched set uint[2048] | frame table uint[2 * HC] | frame slots int[HC] | key list
// int[HC] | row scratch int[4][max_gt] (A_g, partner key + 1, I, A_p) | row state int[4][max_gt] (last key + 1, gap, present, tracked)
struct MotsWs {
    int *hdr;
    unsigned *kbits, *ftab;
    int *fslots, *klist, *r_ag, *r_key, *r_i, *r_ap, *last, *gap, *present, *tracked;
    int fbits;
};

static inline size_t mots_ws_ints(int bits, int max_gt) { return 16 + MOTS_KBITS + 4 * ((size_t)1 << bits) + 8 * (size_t)max_gt; }

static inline MotsWs mots_ws(void *base, int max_gt, long npix)
{
    MotsWs w;
    w.fbits = pan_frame_bits(npix);
    const size_t HC = (size_t)1 << w.fbits;
    int *p = (int *)base;
    w.hdr = p;
    p += 16;
    w.kbits = (unsigned *)p;
    p += MOTS_KBITS;
    w.ftab = (unsigned *)p;
    p += 2 * HC;
    w.fslots = p;
    p += HC;
    w.klist = p;
    p += HC;
    w.r_ag = p;
    w.r_key = p + max_gt;
    w.r_i = p + 2 * (size_t)max_gt;
    w.r_ap = p + 3 * (size_t)max_gt;
    p += 4 * (size_t)max_gt;
    w.last = p;
    w.gap = p + max_gt;
    w.present = p + 2 * (size_t)max_gt;
    w.tracked = p + 3 * (size_t)max_gt;
    return w;
}

// count v > 0 of one cell of the frame: the workgroup's LDS table, or the frame table when that is full around the cell's slot
__device__ static inline void mots_lds_add(unsigned *s_key, int *s_val, const MotsWs &ws, int *counter, unsigned long long *status,
                                           const unsigned cell, const int v)
{
    if (!pan_lds_count<PQ_HASH_BITS>(s_key, s_val, cell, v))   // LDS table full around this slot
        pan_table_add(ws.ftab, ws.fbits, ws.fslots, counter, status, MOTS_FULL_FRAME, cell, (unsigned)v);
}

// one run of `run` pixels with the same pred key and GT id
__device__ static inline void mots_flush(unsigned *s_key, int *s_val, const MotsWs &ws, int *counter, unsigned long long *status,
                                         const int *s_id, const int *s_info, const unsigned char *s_cat, const int n, const unsigned pk,
                                         const int gid, const int run)
{
    const int g = gid == 0 ? -1 : pq_find(s_id, n, gid);      // ids not in the sequence table are ignored, like 0
    const unsigned c = pk >> 8;
    const bool pred = c != 255 && s_cat[c] != MOTS_CAT_KNOWN;  // a thing key, or one of an unknown category (which is reported)
    const int info = g >= 0 ? s_info[g] : 0;
    if (pred) {
        mots_lds_add(s_key, s_val, ws, counter, status, MOTS_KIND(MOTS_AREA_P) | pk, run);
        if (g < 0 || ((info & MOTS_ROW_CROWD) && (unsigned)(info & 255) == c))
            mots_lds_add(s_key, s_val, ws, counter, status, MOTS_KIND(MOTS_IGN) | pk, run);
    }
    if (g >= 0 && (info & (MOTS_ROW_CROWD | MOTS_ROW_THING)) == MOTS_ROW_THING) {
        mots_lds_add(s_key, s_val, ws, counter, status, MOTS_KIND(MOTS_AREA_G) | (unsigned)g, run);
        if (pred && (unsigned)(info & 255) == c) mots_lds_add(s_key, s_val, ws, counter, status, MOTS_KIND(MOTS_JOINT) | (unsigned)g << 16 | pk, run);
    }
}

// table: int[2 * n] rows in ascending id (id, category | crowd << 8 | thing << 9)
__global__ void __launch_bounds__(256)
mots_hist_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ gt, const long npix, const bool vec,
                 const int *__restrict__ table, const int n, const unsigned char *__restrict__ cat_info, MotsWs ws, const int par,
                 unsigned long long *__restrict__ status)
{
    extern __shared__ unsigned s_hist[];
    __shared__ unsigned char s_cat[256];
    unsigned *s_key = s_hist;
    int *s_val = (int *)(s_hist + PQ_HASH);
    int *s_id = (int *)(s_hist + 2 * PQ_HASH);
    int *s_info = s_id + n;
    const int t = threadIdx.x;
    pan_lds_clear<PQ_HASH_BITS>(s_key, s_val, 1);
    for (int i = t; i < n; i += blockDim.x) { s_id[i] = table[2 * i]; s_info[i] = table[2 * i + 1]; }
    s_cat[t] = cat_info[t];
    __syncthreads();
    int *counter = &ws.hdr[par];
    const long p0 = ((long)blockIdx.x * blockDim.x + t) * PAN_RUN;
    if (p0 < npix)
        pan_pair_walk<false>(pred, gt, nullptr, p0, npix, vec, [&](const unsigned pk, const int gid, unsigned, const int run) {
            mots_flush(s_key, s_val, ws, counter, status, s_id, s_info, s_cat, n, pk, gid, run);
        });
    __syncthreads();
    pan_lds_drain<PQ_HASH_BITS>(s_key, [&](const unsigned k, const int i) {
        pan_table_add(ws.ftab, ws.fbits, ws.fslots, counter, status, MOTS_FULL_FRAME, k, (unsigned)s_val[i]);
    });
}

// the frame's cells: matches into the row scratch and the matched set, keys into the key list; the table is only read
__global__ void __launch_bounds__(256)
mots_match_kernel(MotsWs ws, const int nrows, const int par, const unsigned char *__restrict__ cat_info, const long long where,
                  unsigned long long *__restrict__ status)
{
    const int cap = 1 << ws.fbits;
    const int n = min(max(ws.hdr[par], 0), cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {   // the lists of the frame before: its last reader ended with the launch before
        ws.hdr[par ^ 1] = 0;
        ws.hdr[2 + (par ^ 1)] = 0;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int slot = ws.fslots[i] & (cap - 1);
        const unsigned k = ws.ftab[2 * slot], v = ws.ftab[2 * slot + 1];
        if (k == 0) continue;   // (only a slot list that was not zero to begin with)
        const unsigned cell = k - 1, kind = cell >> 28;
        if (kind == MOTS_AREA_G) {
            const int row = cell & 0xfff;
            if (row < nrows) ws.r_ag[row] = (int)v;
        } else if (kind == MOTS_JOINT) {
            const int row = (cell >> 16) & 0xfff;
            const unsigned pk = cell & 0xffff;
            if (row >= nrows) continue;
            const unsigned ap = pan_table_lookup(ws.ftab, ws.fbits, MOTS_KIND(MOTS_AREA_P) | pk);
            const unsigned ag = pan_table_lookup(ws.ftab, ws.fbits, MOTS_KIND(MOTS_AREA_G) | (unsigned)row);
            if (3ll * (long long)v > (long long)ag + (long long)ap) {   // at most one key per row and one row per key: plain stores
                ws.r_key[row] = (int)pk + 1;
                ws.r_i[row] = (int)v;
                ws.r_ap[row] = (int)ap;
                atomicOr(&ws.kbits[pk >> 5], 1u << (pk & 31));
            }
        } else if (kind == MOTS_AREA_P) {
            const unsigned pk = cell & 0xffff;
            if (!(cat_info[pk >> 8] & MOTS_CAT_KNOWN))
                atomicMin(status + 1, (unsigned long long)(where | (long long)(pk >> 8)));   // the first frame, its lowest category
            const unsigned ign = pan_table_lookup(ws.ftab, ws.fbits, MOTS_KIND(MOTS_IGN) | pk);
            const int pos = atomicAdd(&ws.hdr[2 + par], 1);
            if (pos >= 0 && pos < cap) ws.klist[pos] = (int)(pk | (2ll * (long long)ign > (long long)v ? 0x10000u : 0u) | 0x20000u);
        }
    }
}

// counts: int64 [MOTS_COUNTS][256]; soft: double [256]
__global__ void __launch_bounds__(MOTS_T)
mots_state_kernel(MotsWs ws, const int *__restrict__ table, const int nrows, const int par, int64_t *__restrict__ counts,
                  double *__restrict__ soft)
{
    extern __shared__ __attribute__((aligned(16))) double s_iou[];   // [nrows] | int s_flag[nrows]
    const int t = threadIdx.x;
    const int cap = 1 << ws.fbits;
    if (blockIdx.x > 0) {
        const int tid = (blockIdx.x - 1) * blockDim.x + t, step = (gridDim.x - 1) * blockDim.x;
        const int nk = min(max(ws.hdr[2 + par], 0), cap), n = min(max(ws.hdr[par], 0), cap);
        unsigned long long *c64 = (unsigned long long *)counts;
        for (int i = tid; i < nk; i += step) {
            const unsigned e = (unsigned)ws.klist[i];
            ws.klist[i] = 0;
            if (!(e & 0x20000u)) continue;
            const unsigned pk = e & 0xffff, bit = 1u << (pk & 31);
            if (ws.kbits[pk >> 5] & bit) atomicAnd(&ws.kbits[pk >> 5], ~bit);   // matched: no other thread reads this key's bit
            else atomicAdd(&c64[((e & 0x10000u) ? MOTS_FP_IGN : MOTS_FP) * 256 + (pk >> 8)], 1ull);
        }
        for (int i = tid; i < n; i += step) {
            const int slot = ws.fslots[i] & (cap - 1);
            ws.ftab[2 * slot] = 0;
            ws.ftab[2 * slot + 1] = 0;
            ws.fslots[i] = 0;
        }
        return;
    }
    int *s_flag = (int *)(s_iou + nrows);
    for (int g = t; g < nrows; g += MOTS_T) {
        const int info = table[2 * g + 1];
        int flag = 511;
        double v = 0.0;
        if ((info & (MOTS_ROW_CROWD | MOTS_ROW_THING)) == MOTS_ROW_THING) {
            flag = info & 255;
            const int ag = ws.r_ag[g], key = ws.r_key[g];
            if (ag > 0) {
                flag |= MOTS_F_PRESENT;
                ws.present[g] += 1;
                const int last = ws.last[g];
                if (key) {
                    const int inter = ws.r_i[g];
                    v = (double)inter / (double)((long long)ag + (long long)ws.r_ap[g] - (long long)inter);
                    flag |= MOTS_F_MATCHED;
                    ws.tracked[g] += 1;
                    if (last && last != key) flag |= MOTS_F_IDS;
                    ws.last[g] = key;
                    if (ws.gap[g]) {
                        flag |= MOTS_F_FRAG;
                        ws.gap[g] = 0;
                    }
                } else if (last) {
                    ws.gap[g] = 1;
                }
            }
        }
        ws.r_ag[g] = 0;
        ws.r_key[g] = 0;
        ws.r_i[g] = 0;
        ws.r_ap[g] = 0;
        s_flag[g] = flag;
        s_iou[g] = v;
    }
    __syncthreads();
    if (t < 256) {
        // per category, the frame's rows in ascending row (= GT id) order straight into the running sums
        const int c = t;
        double acc = soft[c];
        long long tp = 0, fn = 0, ids = 0, frag = 0;
        for (int g = 0; g < nrows; ++g) {
            const int f = s_flag[g];
            if ((f & 511) != c || !(f & MOTS_F_PRESENT)) continue;
            if (f & MOTS_F_MATCHED) {
                acc += s_iou[g];
                ++tp;
                ids += (f & MOTS_F_IDS) != 0;
                frag += (f & MOTS_F_FRAG) != 0;
            } else {
                ++fn;
            }
        }
        soft[c] = acc;
        counts[MOTS_TP * 256 + c] += tp;
        counts[MOTS_FN * 256 + c] += fn;
        counts[MOTS_GT * 256 + c] += tp + fn;
        counts[MOTS_IDS * 256 + c] += ids;
        counts[MOTS_FRAG * 256 + c] += frag;
    }
}

// MT / PT / ML of every row that was present, mtl int64 [3][256]; all of the workspace zero afterwards
__global__ void __launch_bounds__(256)
mots_end_kernel(MotsWs ws, const int *__restrict__ table, const int nrows, const int max_gt, int64_t *__restrict__ mtl)
{
    const int tid = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    unsigned long long *m64 = (unsigned long long *)mtl;
    for (int g = tid; g < max_gt; g += step) {
        if (g < nrows) {
            const long long p = ws.present[g], tr = ws.tracked[g];
            if (p > 0) {
                const int which = 5 * tr > 4 * p ? 0 : (5 * tr < p ? 2 : 1);
                atomicAdd(&m64[which * 256 + (table[2 * g + 1] & 255)], 1ull);
            }
        }
        ws.last[g] = 0;
        ws.gap[g] = 0;
        ws.present[g] = 0;
        ws.tracked[g] = 0;
    }
    for (int i = tid; i < MOTS_KBITS; i += step) ws.kbits[i] = 0;   // (only bits a full table left behind)
    if (tid < 16) ws.hdr[tid] = 0;
}

extern "C" size_t upsnet_mots_eval_workspace_bytes(int max_gt, int height, int width)
{
    if (max_gt < 0 || max_gt > PQ_MAX_GT || height <= 0 || width <= 0 || (long)height * width > (1L << 24)) return 0;
    return mots_ws_ints(pan_frame_bits((long)height * width), max_gt) * sizeof(int);
}

extern "C" int upsnet_mots_eval_frame(void *stream, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height, int width,
                                      const int *table, int num_rows, int max_gt, int frame, int sequence, const unsigned char *cat_info,
                                      void *workspace, int64_t *counts, double *soft, uint64_t *status)
{
    UPS_REQUIRE(pred_2ch && gt_rgb && cat_info && workspace && counts && soft && status && (table || num_rows == 0), "mots_eval_frame: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "mots_eval_frame: bad frame size %d x %d", height, width);
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PQ_MAX_GT, "mots_eval_frame: max_gt %d outside 0..%d", max_gt, PQ_MAX_GT);
    UPS_REQUIRE(num_rows >= 0 && num_rows <= max_gt, "mots_eval_frame: %d GT rows, more than max_gt %d", num_rows, max_gt);
    UPS_REQUIRE(frame >= 0 && frame < (1 << 24), "mots_eval_frame: frame %d outside 0..2^24-1", frame);
    UPS_REQUIRE(sequence >= 0 && sequence < (1 << 30), "mots_eval_frame: sequence %d outside 0..2^30-1", sequence);
    UPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "mots_eval_frame: workspace not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)height * width;
    const MotsWs ws = mots_ws(workspace, max_gt, npix);
    unsigned long long *stat = (unsigned long long *)status;
    const bool vec = (((uintptr_t)pred_2ch | (uintptr_t)gt_rgb) & 15) == 0;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const int par = frame & 1;
    hipLaunchKernelGGL(mots_hist_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), (size_t)(2 * PQ_HASH + 2 * num_rows) * sizeof(int), st,
                       pred_2ch, gt_rgb, npix, vec, table, num_rows, cat_info, ws, par, stat);
    UPS_CHECK_LAUNCH("mots_hist_kernel");
    const long long where = (long long)sequence << 32 | (long long)frame << 8;
    const int blocks = min(64, 1 << (ws.fbits - 8));
    hipLaunchKernelGGL(mots_match_kernel, dim3(blocks), dim3(256), 0, st, ws, num_rows, par, cat_info, where, stat);
    UPS_CHECK_LAUNCH("mots_match_kernel");
    hipLaunchKernelGGL(mots_state_kernel, dim3(1 + blocks / 4), dim3(MOTS_T), (size_t)num_rows * (sizeof(double) + sizeof(int)), st, ws, table,
                       num_rows, par, counts, soft);
    UPS_CHECK_LAUNCH("mots_state_kernel");
    return 0;
}

extern "C" int upsnet_mots_eval_end(void *stream, int height, int width, const int *table, int num_rows, int max_gt, void *workspace,
                                    int64_t *mtl)
{
    UPS_REQUIRE(workspace && mtl && (table || num_rows == 0), "mots_eval_end: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "mots_eval_end: bad frame size %d x %d", height, width);
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PQ_MAX_GT, "mots_eval_end: max_gt %d outside 0..%d", max_gt, PQ_MAX_GT);
    UPS_REQUIRE(num_rows >= 0 && num_rows <= max_gt, "mots_eval_end: %d GT rows, more than max_gt %d", num_rows, max_gt);
    UPS_REQUIRE(((uintptr_t)workspace & 7) == 0, "mots_eval_end: workspace not 8-byte aligned");
    const MotsWs ws = mots_ws(workspace, max_gt, (long)height * width);
    hipLaunchKernelGGL(mots_end_kernel, dim3(16), dim3(256), 0, (hipStream_t)stream, ws, table, num_rows, max_gt, mtl);
    UPS_CHECK_LAUNCH("mots_end_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------- RLE transitions of a 2-channel map
// A thing segment is a key c << 8 | i with c != 255 and i >= 1 (as in pan_track.hip). In the column-major flattening (position p = x * H
// + y, the wrap from one column's last pixel to the next column's first being adjacent) the membership of a key changes at p iff the
// pixel at p and the one at p - 1 (none before p = 0) differ and one of them is the key's. One thread per pixel in ROW-major order, so
// both loads coalesce; a workgroup reserves its pairs with one global atomic.
__device__ static inline unsigned mots_thing_key(const unsigned char *__restrict__ pan, const long pix)
{
    const unsigned c = pan[3 * pix], i = pan[3 * pix + 1];
    return c != 255 && i != 0 ? (c << 8 | i) : 0xffffffffu;
}

__global__ void __launch_bounds__(256)
pan_rle_transitions_kernel(const unsigned char *__restrict__ pan, const int H, const int W, const int cap, long long *__restrict__ pairs,
                           int *__restrict__ count)
{
    __shared__ int s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const long npix = (long)H * W, pix = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long long e0 = -1, e1 = -1;
    int mine = 0, at = 0;
    if (pix < npix) {
        const int y = (int)(pix / W), x = (int)(pix - (long)y * W);
        const long p = (long)x * H + y;
        const unsigned cur = mots_thing_key(pan, pix);
        unsigned prev = 0xffffffffu;
        if (y > 0) prev = mots_thing_key(pan, pix - W);
        else if (x > 0) prev = mots_thing_key(pan, (long)(H - 1) * W + x - 1);
        if (cur != prev) {
            if (prev != 0xffffffffu) e0 = (long long)prev << 24 | p;
            if (cur != 0xffffffffu) (e0 < 0 ? e0 : e1) = (long long)cur << 24 | p;
            mine = (e0 >= 0) + (e1 >= 0);
            at = atomicAdd(&s_n, mine);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n > 0) s_base = atomicAdd(count, s_n);   // the count is kept even beyond cap: the caller grows and retries
    __syncthreads();
    if (mine) {
        const long pos = (long)s_base + at;
        if (pos >= 0 && pos < cap) pairs[pos] = e0;
        if (mine == 2 && pos + 1 >= 0 && pos + 1 < cap) pairs[pos + 1] = e1;
    }
}

extern "C" int upsnet_pan_rle_transitions(void *stream, const unsigned char *pan_2ch, int height, int width, int cap, int64_t *pairs,
                                          int *count)
{
    UPS_REQUIRE(pan_2ch && count && (pairs || cap == 0), "pan_rle_transitions: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "pan_rle_transitions: bad map size %d x %d", height, width);
    UPS_REQUIRE(cap >= 0, "pan_rle_transitions: cap %d < 0", cap);
    hipStream_t st = (hipStream_t)stream;
    UPS_CHECK_HIP(hipMemsetAsync(count, 0, sizeof(int), st));
    const long npix = (long)height * width;
    hipLaunchKernelGGL(pan_rle_transitions_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, pan_2ch, height, width, cap,
                       (long long *)pairs, count);
    UPS_CHECK_LAUNCH("pan_rle_transitions_kernel");
    return 0;
}
