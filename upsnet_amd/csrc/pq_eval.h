// pq_eval.h -- what pq_eval.hip and pq_boundary.hip share (and video_eval.hip / mots_eval.hip borrow: the limits and pq_find): the
// workspace layout, the count cells behind the pixel pass of pan_pixels.h, the GT preparation kernel and the mask IoU of a pair.
#pragma once
#include "common.h"
#include "pan_pixels.h"

#define PQ_KEYS 65536            // pred keys (cat << 8 | inst); cat 255 = VOID never counted
#define PQ_VOID_OFF PQ_KEYS      // inter(GT VOID, pred key)
#define PQ_JOINT_OFF (2 * PQ_KEYS)
#define PQ_MAX_GT 4096
#define PQ_HASH_BITS 11          // the pixel pass's LDS table: 2048 cells per workgroup
#define PQ_HASH (1 << PQ_HASH_BITS)

struct PqSeg {
    int id, cat, crowd, pad;
    long long area;              // the JSON area (not recounted, as in the reference)
};

// Workspace layout (bytes): int cnt[cnt_cells] (pq_cnt_cells(max_gt) = 2 * PQ_KEYS + max_gt * 256; Boundary PQ appends a second area) | PqSeg seg[max_gt] | double row_iou[max_gt] | int crowd_row[256]
// | int nkeys[2] | int keys[PQ_KEYS] (the image's pred keys with a non-zero area, in arrival order)
struct PqWs {
    int *cnt;
    PqSeg *seg;
    double *row_iou;
    int *crowd_row;
    int *nkeys;
    int *keys;
};

static inline size_t pq_cnt_cells(int max_gt) { return (size_t)2 * PQ_KEYS + (size_t)max_gt * 256; }

static inline PqWs pq_ws(void *base, size_t cnt_cells, int max_gt)
{
    PqWs w;
    char *p = (char *)base;
    w.cnt = (int *)p;
    p += cnt_cells * sizeof(int);
    w.seg = (PqSeg *)p;
    p += (size_t)max_gt * sizeof(PqSeg);
    w.row_iou = (double *)p;
    p += (size_t)max_gt * sizeof(double);
    w.crowd_row = (int *)p;
    w.nkeys = w.crowd_row + 256;
    w.keys = w.nkeys + 2;
    return w;
}

// (static: each translation unit that launches it carries its own copy -- the library is built without relocatable device code)
static __global__ void __launch_bounds__(1024)
pq_prep_kernel(const int64_t *__restrict__ segments, const int n, PqWs ws)
{
    extern __shared__ int s_dyn[];
    int *s_id = s_dyn, *s_rank = s_dyn + n;
    __shared__ int s_last[256];
    const int t = threadIdx.x;
    for (int i = t; i < n; i += blockDim.x) s_id[i] = (int)segments[4 * i];
    for (int c = t; c < 256; c += blockDim.x) s_last[c] = -1;
    __syncthreads();
    for (int i = t; i < n; i += blockDim.x) {
        const int id = s_id[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const int v = s_id[j];
            r += (v < id) | ((v == id) & (j < i));   // ties by JSON position: a permutation even for duplicate ids (refused on the host)
        }
        s_rank[i] = r;
        const int64_t c64 = segments[4 * i + 1];
        const int cat = c64 >= 0 && c64 < 255 ? (int)c64 : 255;   // in bounds whatever the caller passed (the host refuses these)
        PqSeg s;
        s.id = id;
        s.cat = cat;
        s.crowd = segments[4 * i + 2] == 1;
        s.pad = 0;
        s.area = segments[4 * i + 3];
        ws.seg[r] = s;
        if (s.crowd) atomicMax(&s_last[cat], i);
    }
    __syncthreads();
    for (int c = t; c < 256; c += blockDim.x) ws.crowd_row[c] = s_last[c] >= 0 ? s_rank[s_last[c]] : -1;
}

// global count of one cell (v > 0): the first arrival at a pred area cell appends its key to the list
__device__ static inline void pq_global_add(const PqWs &ws, const unsigned cell, const int v)
{
    const int old = atomicAdd(&ws.cnt[cell], v);
    if (cell < PQ_KEYS && old == 0) {
        const int pos = atomicAdd(ws.nkeys, 1);
        if (pos < PQ_KEYS) ws.keys[pos] = (int)cell;   // at most 255 * 256 keys per image: always true for a zeroed workspace
    }
}

__device__ static inline void pq_add(unsigned *s_key, int *s_val, const PqWs &ws, const unsigned cell, const int v)
{
    if (!pan_lds_count<PQ_HASH_BITS>(s_key, s_val, cell, v)) pq_global_add(ws, cell, v);   // LDS table full around this slot
}

__device__ static inline int pq_find(const int *s_id, const int n, const int id)
{
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int v = s_id[mid];
        if (v == id) return mid;
        if (v < id) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

// one run of `run` pixels with the same pred key (cat << 8 | inst) and GT id
__device__ static inline void pq_flush(unsigned *s_key, int *s_val, const PqWs &ws, const int *s_id, const unsigned char *s_cat,
                                       const int n, const unsigned pk, const int gid, const int run)
{
    const unsigned cat = pk >> 8;
    if (cat == 255) return;                                      // pred VOID, whatever its instance
    pq_add(s_key, s_val, ws, pk, run);                          // pred area = pixel count
    if (gid == 0) {
        pq_add(s_key, s_val, ws, PQ_VOID_OFF + pk, run);
    } else {
        const int g = pq_find(s_id, n, gid);                     // ids not in segments_info take part in nothing
        if (g >= 0 && s_cat[g] == cat) pq_add(s_key, s_val, ws, PQ_JOINT_OFF + (unsigned)g * 256 + (pk & 255), run);
    }
}

#define PQM_T 1024
#define PQM_WAVES (PQM_T / UPS_WAVE)

// iou of GT row g (category cat, JSON area) with pred instance inst of the same category, exactly as the reference:
// union = area_p + area_g - inter - inter(VOID, p) in integers, iou = inter / union in float64
__device__ static inline double pq_iou(const int *__restrict__ cnt, const long long area_g, const int cat, const int inst, const int inter)
{
    const int k = cat << 8 | inst;
    const long long uni = (long long)cnt[k] + area_g - inter - cnt[PQ_VOID_OFF + k];
    return (double)inter / (double)uni;
}
