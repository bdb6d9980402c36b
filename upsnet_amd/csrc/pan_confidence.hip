// pan_confidence.hip -- what the panoptic confidence plane (panoptic.hip: panoptic_fuse_up_conf_kernel) says about
// the segments of a 2-channel map: a score per segment, and the removal of the doubtful ones. The reference has neither; the rules
// are this project's own, stated in include/upsnet_hip.h and restated in plain numpy in tests/pan_confidence_ref.py.
//   pcf_count_kernel    the pixel pass of pan_pixels.h: 16 pixels of the map (pan_load48) and their 16 confidence bytes (pan_load16)
//                       per thread, runs of one key in registers, an LDS table per workgroup with two payload planes (area, sum of
//                       the confidence bytes), the global fallback when the table is full around a key, then one global add per plane,
//                       distinct key and workgroup. VOID (category 255) is no segment and is not counted.
//   pcf_compact_kernel  one workgroup: the keys that have pixels, in ascending key, as rows (key, area, sum_q).
//   pcf_filter_kernel   one pass: every pixel of a segment whose row says sum_q < T * 255 * area becomes VOID (255, 0, 0); a run's row is
//                       found by bisection in the table.
// Integer atomics only, and the filter's comparison is two exact conversions and one IEEE double product: the same map and plane give
// the same bytes on every run, and the bytes numpy gives.
#include "common.h"
#include "upsnet_hip.h"
#include "pan_pixels.h"

#define PCF_HASH_BITS 10          // the count pass's LDS table: 1024 keys per workgroup, two planes
#define PCF_HASH (1 << PCF_HASH_BITS)
#define PCF_MAX_SEGMENTS 65280    // 255 categories x 256 instances
#define PCF_HEAD 4                // uints before the first table row: [0] = number of rows
#define PCF_ROW 3                 // uints per row: key, area, sum_q
#define PCF_T 1024
#define PCF_PER (PAN_KEYS / PCF_T)

__device__ static inline void pcf_add(unsigned *s_key, unsigned *s_val, unsigned *cells, const unsigned key, const unsigned run, const unsigned sq)
{
    if ((key >> 8) == 255) return;
    const bool held = pan_lds_claim<PCF_HASH_BITS>(s_key, key, [&](const unsigned slot) {
        atomicAdd(&s_val[slot], run);
        atomicAdd(&s_val[PCF_HASH + slot], sq);
    });
    if (!held) {
        atomicAdd(&cells[key], run);
        atomicAdd(&cells[PAN_KEYS + key], sq);
    }
}

// cells: uint [2][PAN_KEYS] = area | sum_q, zero on entry
__global__ void __launch_bounds__(256)
pcf_count_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ conf, const long npix, const bool vec_pred,
                 const bool vec_conf, unsigned *__restrict__ cells)
{
    __shared__ unsigned s_key[PCF_HASH];
    __shared__ unsigned s_val[2 * PCF_HASH];
    pan_lds_clear<PCF_HASH_BITS>(s_key, s_val, 2);
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 < npix) {
        unsigned w[12], c[4];
        pan_load48(pred, p0, npix, vec_pred, w);
        pan_load16(conf, p0, npix, vec_conf, c);
        unsigned pk = 0, run = 0, sq = 0;
#pragma unroll
        for (int i = 0; i < PAN_RUN; ++i) {
            if (p0 + i < npix) {
                const unsigned k = pan_byte(w, 3 * i) << 8 | pan_byte(w, 3 * i + 1);
                if (k != pk) {
                    if (run) pcf_add(s_key, s_val, cells, pk, run, sq);
                    pk = k;
                    run = 0;
                    sq = 0;
                }
                ++run;
                sq += pan_byte(c, i);
            }
        }
        if (run) pcf_add(s_key, s_val, cells, pk, run, sq);
    }
    __syncthreads();
    pan_lds_drain<PCF_HASH_BITS>(s_key, [&](const unsigned k, const int i) {
        atomicAdd(&cells[k], s_val[i]);
        atomicAdd(&cells[PAN_KEYS + k], s_val[PCF_HASH + i]);
    });
}

// table: [0] = number of rows n, [1..3] = 0, then n rows (key, area, sum_q) in ascending key; rows past n are not written
__global__ void __launch_bounds__(PCF_T)
pcf_compact_kernel(const unsigned *__restrict__ cells, unsigned *__restrict__ table)
{
    __shared__ int s_scan[2][PCF_T];
    const int t = threadIdx.x;
    int mine = 0;
    for (int j = 0; j < PCF_PER; ++j) mine += cells[t * PCF_PER + j] != 0;
    s_scan[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < PCF_T; d <<= 1) {   // inclusive scan
        s_scan[cur ^ 1][t] = s_scan[cur][t] + (t >= d ? s_scan[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int pos = s_scan[cur][t] - mine;
    for (int j = 0; j < PCF_PER; ++j) {
        const unsigned key = (unsigned)(t * PCF_PER + j), a = cells[key];
        if (a == 0) continue;
        unsigned *row = table + PCF_HEAD + (size_t)pos * PCF_ROW;   // (VOID keys hold no count: pos < PCF_MAX_SEGMENTS)
        row[0] = key;
        row[1] = a;
        row[2] = cells[PAN_KEYS + key];
        ++pos;
    }
    if (t < PCF_HEAD) table[t] = t == 0 ? (unsigned)s_scan[cur][PCF_T - 1] : 0u;
}

__global__ void __launch_bounds__(256)
pcf_filter_kernel(const unsigned char *pred, unsigned char *out, const long npix, const bool vec, const unsigned *__restrict__ table,
                  const double min_score)
{
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    const int n = (int)min(table[0], (unsigned)PCF_MAX_SEGMENTS);
    const unsigned *rows = table + PCF_HEAD;
    unsigned w[12];
    pan_load48(pred, p0, npix, vec, w);
    unsigned pk = 0xffffffffu;
    bool drop = false;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        const unsigned k = pan_byte(w, 3 * i) << 8 | pan_byte(w, 3 * i + 1);   // (pixels past the end read as key 0 and are not stored)
        if (k != pk) {
            pk = k;
            drop = false;
            if ((k >> 8) != 255) {
                int lo = 0, hi = n - 1;
                while (lo <= hi) {
                    const int mid = (lo + hi) >> 1;
                    const unsigned v = rows[(size_t)mid * PCF_ROW];
                    if (v == k) {
                        drop = (double)rows[(size_t)mid * PCF_ROW + 2] < min_score * (double)(255u * rows[(size_t)mid * PCF_ROW + 1]);
                        break;
                    }
                    if (v < k) lo = mid + 1;
                    else hi = mid - 1;
                }
            }
        }
        if (drop) {
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                const int j = 3 * i + b;
                w[j >> 2] = (w[j >> 2] & ~(255u << (8 * (j & 3)))) | ((b == 0 ? 255u : 0u) << (8 * (j & 3)));
            }
        }
    }
    pan_store48(out, p0, npix, vec, w);
}

extern "C" size_t upsnet_pan_segment_scores_workspace_bytes(void) { return (size_t)2 * PAN_KEYS * sizeof(unsigned); }

extern "C" size_t upsnet_pan_segment_scores_table_ints(void) { return (size_t)PCF_HEAD + (size_t)PCF_MAX_SEGMENTS * PCF_ROW; }

extern "C" int upsnet_pan_segment_scores(void *stream, const unsigned char *pan_2ch, const unsigned char *conf, int height, int width,
                                         void *workspace, unsigned *table)
{
    UPS_REQUIRE(pan_2ch && conf && workspace && table, "pan_segment_scores: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "pan_segment_scores: a map of %d x %d pixels: H * W must lie in 1..2^24",
                height, width);
    UPS_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)table & 3) == 0, "pan_segment_scores: workspace / table not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned *cells = (unsigned *)workspace;
    if (ups_zero_async(cells, upsnet_pan_segment_scores_workspace_bytes(), st)) return 1;
    const long npix = (long)height * width;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    hipLaunchKernelGGL(pcf_count_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, pan_2ch, conf, npix,
                       ((uintptr_t)pan_2ch & 15) == 0, ((uintptr_t)conf & 15) == 0, cells);
    UPS_CHECK_LAUNCH("pcf_count_kernel");
    hipLaunchKernelGGL(pcf_compact_kernel, dim3(1), dim3(PCF_T), 0, st, cells, table);
    UPS_CHECK_LAUNCH("pcf_compact_kernel");
    return 0;
}

extern "C" int upsnet_pan_score_filter(void *stream, const unsigned char *pan_2ch, int height, int width, const unsigned *table,
                                       double min_score, unsigned char *out_2ch)
{
    UPS_REQUIRE(pan_2ch && table && out_2ch, "pan_score_filter: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= (1L << 24), "pan_score_filter: a map of %d x %d pixels: H * W must lie in 1..2^24",
                height, width);
    UPS_REQUIRE(min_score >= 0.0 && min_score <= 1.0, "pan_score_filter: min_score %g outside 0..1", min_score);
    UPS_REQUIRE(((uintptr_t)table & 3) == 0, "pan_score_filter: table not 4-byte aligned");
    const long npix = (long)height * width;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    hipLaunchKernelGGL(pcf_filter_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pan_2ch, out_2ch, npix,
                       (((uintptr_t)pan_2ch | (uintptr_t)out_2ch) & 15) == 0, table, min_score);
    UPS_CHECK_LAUNCH("pcf_filter_kernel");
    return 0;
}
