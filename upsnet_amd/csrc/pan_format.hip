// pan_format.hip -- the COCO panoptic format on the device, both directions:
//   * 2-channel prediction (category, instance) -> panoptic PNG content plus its segment table: _converter_2ch_single_core of the
//     reference (upsnet/dataset/base_dataset.py:463-511, without vis_panoptic);
//   * panoptic PNG of arbitrary 24-bit ids plus the JSON's segments -> 2-channel map, so that pq_eval.hip scores any COCO-panoptic
//     prediction (the general form of _pq_compute_single_core, :514-608, with its two sanity checks :531-542).
//
// Reference (numpy, host): np.unique over 1000 * ch0 + ch1, then per segment a full-image mask for its colour, area and bbox.
// Here, integers only, three launches per image and a workspace that every call leaves zeroed:
//   pan_seg_kernel     the pixel pass of pan_pixels.h with the row walk (a run ends with its key or its row) and the bbox payload: an
//                      LDS table per workgroup, then per distinct key and workgroup one global atomic add (area) and four atomic max
//                      (x_max, y_max, INV - x_min, INV - y_min: a zeroed cell is "nothing yet" for all five). A full LDS table
//                      falls back to the global atomics, so a pixel-noise map with all 65280 keys is still exact.
//   pan_color_kernel   one workgroup: compacts the non-empty keys in ascending key (np.unique's order) into the output table, gives
//                      every segment its colour (the rule below; one thread, a bitmap of the 2^24 colours for "taken"), fills the
//                      key -> colour table for the paint pass, and clears every cell and bit it used.
//   pan_paint_kernel   one pass: RGB of the key's colour, VOID (ch0 == 255) -> (0,0,0).
// Key = ch0 << 8 | ch1, as in pq_eval.hip: the same segments in the same order as the reference's 1000 * ch0 + ch1.
//
// Colour rule (the contract of panopticapi's IdGenerator with its np.random draw replaced by a counter-based sequence). Segments are
// visited in ascending key; `ordinal` counts the segments of one category from 0. The taken set starts as every stuff category's
// colour. The first segment of a category takes the category colour if that is not (0,0,0) and -- for a thing -- not taken. Every other
// segment tries attempt a = 0, 1, ...: cell = (lowbias32(category << 16 | ordinal) + a * 100003) mod 61^3, offset per channel
// (cell mod 61, cell / 61 mod 61, cell / 3721) - 30, colour = clamp(base + offset, 0, 255), until the colour is neither (0,0,0) nor
// taken. 100003 is coprime to 61^3, so the 226981 attempts visit every cell of the +-30 cube once.
#include "common.h"
#include "upsnet_hip.h"
#include "pan_pixels.h"

#define PF_KEYS 65536
#define PF_MAX_SEGMENTS 65280     // 255 categories x 256 instances
#define PF_HASH_BITS 10           // the segment pass's LDS table: 1024 keys per workgroup, five planes
#define PF_HASH (1 << PF_HASH_BITS)
#define PF_CUBE 226981u           // 61^3 offsets of the +-30 cube
#define PF_STEP 100003u
#define PF_TAKEN_WORDS (1 << 19)  // one bit per 24-bit colour
#define PF_HEAD 8                 // ints before the first table row
#define PF_ROW 8                  // ints per row: key, area, x_min, y_min, x_max, y_max, colour (= id), ordinal within the category
#define PF_RELABEL_LDS 4096       // segments whose table (and counters) the relabel kernel keeps in LDS
#define PF_INV62 (1ull << 62)

// Workspace (ints): area | INV - x_min | INV - y_min | x_max | y_max (the five planes of pan_pixels.h's bbox payload, from `area`) |
// colour, each [PF_KEYS], then the taken bitmap
struct PfWs {
    int *area, *nxmin, *nymin, *xmax, *ymax;
    unsigned *color, *taken;
};

static PfWs pf_ws(void *base)
{
    PfWs w;
    int *p = (int *)base;
    w.area = p;
    w.nxmin = p + PF_KEYS;
    w.nymin = p + 2 * PF_KEYS;
    w.xmax = p + 3 * PF_KEYS;
    w.ymax = p + 4 * PF_KEYS;
    w.color = (unsigned *)(p + 5 * PF_KEYS);
    w.taken = (unsigned *)(p + 6 * PF_KEYS);
    return w;
}

__global__ void __launch_bounds__(256)
pan_seg_kernel(const unsigned char *__restrict__ pred, const long npix, const int width, const bool vec, PfWs ws)
{
    __shared__ unsigned s_key[PF_HASH];
    __shared__ int s_val[5 * PF_HASH];
    pan_lds_clear<PF_HASH_BITS>(s_key, s_val, 5);
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 < npix)
        pan_row_walk(pred, p0, npix, width, vec, [&](const unsigned key, const int run, const int x0, const int y) {
            if ((key >> 8) != 255) pan_box_add<PF_HASH_BITS>(s_key, s_val, ws.area, key, run, x0, y);   // VOID, whatever its instance, is no segment
        });
    __syncthreads();
    pan_box_drain<PF_HASH_BITS>(s_key, s_val, ws.area);
}

__host__ __device__ static inline unsigned pf_lowbias32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ static inline unsigned pf_clamp_add(const unsigned base, const int d)
{
    const int v = (int)base + d;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// attempt a of (category, ordinal) around base (R | G << 8 | B << 16)
__device__ static inline unsigned pf_candidate(const unsigned base, const unsigned start, const unsigned a)
{
    const unsigned cell = (unsigned)(((unsigned long long)start + (unsigned long long)a * PF_STEP) % PF_CUBE);
    const int dr = (int)(cell % 61) - 30, dg = (int)(cell / 61 % 61) - 30, db = (int)(cell / 3721) - 30;
    return pf_clamp_add(base & 255, dr) | pf_clamp_add(base >> 8 & 255, dg) << 8 | pf_clamp_add(base >> 16 & 255, db) << 16;
}

#define PFC_T 1024
#define PFC_PER (PF_KEYS / PFC_T)   // 64 keys per thread: a category is 4 threads

// cat_table int [256]: -1 = not in the category table, else colour (R | G << 8 | B << 16) | isthing << 24.
// table: [0] = number of segments, [1] = error (0 none, 1 unknown category, 2 no free colour), [2] = the category of the error
// (the lowest one for error 1), rows from table + PF_HEAD.
__global__ void __launch_bounds__(PFC_T)
pan_color_kernel(const int *__restrict__ cat_table, PfWs ws, int *__restrict__ table)
{
    __shared__ int s_scan[2][PFC_T];
    __shared__ int s_cat[256];
    __shared__ int s_err[2];
    const int t = threadIdx.x;
    if (t < 256) s_cat[t] = cat_table[t];
    if (t < 2) s_err[t] = t == 0 ? 0 : 256;
    int mine = 0;
    for (int j = 0; j < PFC_PER; ++j) mine += ws.area[t * PFC_PER + j] != 0;
    s_scan[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < PFC_T; d <<= 1) {   // inclusive scan
        s_scan[cur ^ 1][t] = s_scan[cur][t] + (t >= d ? s_scan[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int n = s_scan[cur][PFC_T - 1];
    const int cat_first = (t & ~3) ? s_scan[cur][(t & ~3) - 1] : 0;   // segments before this thread's category
    int pos = s_scan[cur][t] - mine;
    // stuff colours are taken from the start (colour 0 is refused by value)
    if (t < 256 && s_cat[t] >= 0 && !(s_cat[t] >> 24 & 1)) {
        const unsigned c = (unsigned)s_cat[t] & 0xffffffu;
        if (c) atomicOr(&ws.taken[c >> 5], 1u << (c & 31));
    }
    for (int j = 0; j < PFC_PER; ++j) {
        const int key = t * PFC_PER + j, a = ws.area[key];
        if (a == 0) continue;
        int *row = table + PF_HEAD + (size_t)pos * PF_ROW;
        row[0] = key;
        row[1] = a;
        row[2] = PAN_INV - ws.nxmin[key];
        row[3] = PAN_INV - ws.nymin[key];
        row[4] = ws.xmax[key];
        row[5] = ws.ymax[key];
        row[6] = 0;
        row[7] = pos - cat_first;
        ws.area[key] = 0;   // the workspace is zero again for the next image
        ws.nxmin[key] = 0;
        ws.nymin[key] = 0;
        ws.xmax[key] = 0;
        ws.ymax[key] = 0;
        ++pos;
    }
    __syncthreads();
    if (t == 0) {
        for (int i = 0; i < n; ++i) {
            int *row = table + PF_HEAD + (size_t)i * PF_ROW;
            const int cat = row[0] >> 8, ordinal = row[7], info = s_cat[cat];
            if (info < 0) {
                s_err[0] = 1;
                s_err[1] = min(s_err[1], cat);
                continue;
            }
            const unsigned base = (unsigned)info & 0xffffffu;
            const bool thing = info >> 24 & 1;
            unsigned c = 0;
            if (ordinal == 0 && base != 0 && (!thing || !(ws.taken[base >> 5] >> (base & 31) & 1))) {
                c = base;
            } else {
                const unsigned start = pf_lowbias32((unsigned)cat << 16 | (unsigned)ordinal) % PF_CUBE;
                for (unsigned a = 0; a < PF_CUBE; ++a) {
                    const unsigned v = pf_candidate(base, start, a);
                    if (v != 0 && !(ws.taken[v >> 5] >> (v & 31) & 1)) { c = v; break; }
                }
                if (c == 0) {
                    if (s_err[0] == 0) { s_err[0] = 2; s_err[1] = cat; }
                    continue;
                }
            }
            ws.taken[c >> 5] |= 1u << (c & 31);
            row[6] = (int)c;
        }
    }
    __syncthreads();
    for (int i = t; i < n; i += PFC_T) {
        const int *row = table + PF_HEAD + (size_t)i * PF_ROW;
        const unsigned c = (unsigned)row[6];
        ws.color[row[0]] = c;
        if (c) atomicAnd(&ws.taken[c >> 5], ~(1u << (c & 31)));
    }
    if (t < 256 && s_cat[t] >= 0 && !(s_cat[t] >> 24 & 1)) {
        const unsigned c = (unsigned)s_cat[t] & 0xffffffu;
        if (c) atomicAnd(&ws.taken[c >> 5], ~(1u << (c & 31)));
    }
    if (t < PF_HEAD) table[t] = t == 0 ? n : (t == 1 ? s_err[0] : (t == 2 && s_err[0] ? s_err[1] : 0));
}

__global__ void __launch_bounds__(256)
pan_paint_kernel(const unsigned char *__restrict__ pred, unsigned char *__restrict__ rgb, const long npix, const bool vec,
                 const unsigned *__restrict__ color)
{
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    unsigned w[12], o[12];
    pan_load48(pred, p0, npix, vec, w);
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = 0;
    unsigned pk = 0xffffffffu, c = 0;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        const unsigned k = pan_byte(w, 3 * i) << 8 | pan_byte(w, 3 * i + 1);   // (pixels past the end read as key 0 and are not stored)
        if (k != pk) {
            pk = k;
            c = (k >> 8) == 255 ? 0u : color[k];
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) o[(3 * i + b) >> 2] |= (c >> (8 * b) & 255u) << (8 * ((3 * i + b) & 3));
    }
    pan_store48(rgb, p0, npix, vec, o);
}

extern "C" size_t upsnet_pan_format_workspace_bytes(void) { return ((size_t)6 * PF_KEYS + PF_TAKEN_WORDS) * sizeof(int); }

extern "C" size_t upsnet_pan_format_table_ints(void) { return (size_t)PF_HEAD + (size_t)PF_MAX_SEGMENTS * PF_ROW; }

extern "C" int upsnet_pan_format(void *stream, const unsigned char *pred_2ch, int height, int width, const int *cat_table, void *workspace,
                                 unsigned char *rgb, int *table)
{
    UPS_REQUIRE(pred_2ch && cat_table && workspace && rgb && table, "pan_format: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "pan_format: bad image size %d x %d", height, width);
    UPS_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)table & 3) == 0, "pan_format: workspace / table not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const PfWs ws = pf_ws(workspace);
    const long npix = (long)height * width;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    hipLaunchKernelGGL(pan_seg_kernel, dim3(grid), dim3(256), 0, st, pred_2ch, npix, width, ((uintptr_t)pred_2ch & 15) == 0, ws);
    UPS_CHECK_LAUNCH("pan_seg_kernel");
    hipLaunchKernelGGL(pan_color_kernel, dim3(1), dim3(PFC_T), 0, st, cat_table, ws, table);
    UPS_CHECK_LAUNCH("pan_color_kernel");
    hipLaunchKernelGGL(pan_paint_kernel, dim3(grid), dim3(256), 0, st, pred_2ch, rgb, npix, (((uintptr_t)pred_2ch | (uintptr_t)rgb) & 15) == 0,
                       ws.color);
    UPS_CHECK_LAUNCH("pan_paint_kernel");
    return 0;
}


// ---------------------------------------------------------------------------------------------
// Relabel: panoptic PNG (id = R + 256 G + 65536 B) -> 2-channel map through the JSON's segments sorted by id, rows (id, category,
// instance slot). Id 0 and ids that are not in the table become VOID (255, 0). Pixels are counted per row; the smallest id that is in
// the PNG, is not 0 and is not in the table is kept in status[0] as the maximum of 2^62 - ((image_index + 1) << 24 | id), so that the
// earliest image wins, then the smallest id, whatever the arrival order.
__device__ static inline int pf_find(const int *ids, const int stride, const int n, const int id)
{
    int lo = 0, hi = n - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        const int v = ids[(size_t)mid * stride];
        if (v == id) return mid;
        if (v < id) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

__global__ void __launch_bounds__(256)
pan_relabel_kernel(const unsigned char *__restrict__ rgb, unsigned char *__restrict__ out, const long npix, const bool vec,
                   const int *__restrict__ table, const int n, const bool use_lds, const int image_index, int *__restrict__ counts,
                   unsigned long long *__restrict__ status)
{
    extern __shared__ int s_rel[];   // use_lds: ids [n] | counts [n] | category << 8 | slot [n]
    int *s_id = s_rel, *s_cnt = s_rel + n, *s_cs = s_rel + 2 * n;
    const int t = threadIdx.x;
    if (use_lds) {
        for (int i = t; i < n; i += blockDim.x) {
            s_id[i] = table[3 * i];
            s_cnt[i] = 0;
            s_cs[i] = (table[3 * i + 1] & 255) << 8 | (table[3 * i + 2] & 255);
        }
        __syncthreads();
    }
    const long p0 = ((long)blockIdx.x * blockDim.x + t) * PAN_RUN;
    if (p0 < npix) {
        unsigned w[12], o[12];
        pan_load48(rgb, p0, npix, vec, w);
#pragma unroll
        for (int j = 0; j < 12; ++j) o[j] = 0;
        int pid = -1, row = -1, run = 0;
        unsigned cs = 255u << 8;
#pragma unroll
        for (int i = 0; i < PAN_RUN; ++i) {
            if (p0 + i < npix) {
                const int id = (int)(pan_byte(w, 3 * i) | pan_byte(w, 3 * i + 1) << 8 | pan_byte(w, 3 * i + 2) << 16);
                if (id != pid) {
                    if (run && row >= 0) atomicAdd(use_lds ? &s_cnt[row] : &counts[row], run);
                    pid = id;
                    run = 0;
                    row = id == 0 ? -1 : (use_lds ? pf_find(s_id, 1, n, id) : pf_find(table, 3, n, id));
                    if (row >= 0) {
                        cs = use_lds ? (unsigned)s_cs[row] : (unsigned)((table[3 * row + 1] & 255) << 8 | (table[3 * row + 2] & 255));
                    } else {
                        cs = 255u << 8;
                        if (id != 0) atomicMax(status, PF_INV62 - ((unsigned long long)(image_index + 1) << 24 | (unsigned)id));
                    }
                }
                ++run;
                o[(3 * i) >> 2] |= (cs >> 8) << (8 * ((3 * i) & 3));
                o[(3 * i + 1) >> 2] |= (cs & 255u) << (8 * ((3 * i + 1) & 3));
            }
        }
        if (run && row >= 0) atomicAdd(use_lds ? &s_cnt[row] : &counts[row], run);
        pan_store48(out, p0, npix, vec, o);
    }
    if (use_lds) {
        __syncthreads();
        for (int i = t; i < n; i += blockDim.x) {
            const int v = s_cnt[i];
            if (v) atomicAdd(&counts[i], v);
        }
    }
}

// a segment of the JSON without a pixel in the PNG: the smallest id of the earliest image, kept in status[1] like status[0]
__global__ void __launch_bounds__(256)
pan_relabel_check_kernel(const int *__restrict__ table, const int n, const int image_index, const int *__restrict__ counts,
                         unsigned long long *__restrict__ status)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && counts[i] == 0)
        atomicMax(status + 1, PF_INV62 - ((unsigned long long)(image_index + 1) << 24 | (unsigned)(table[3 * i] & 0xffffff)));
}

extern "C" int upsnet_pan_relabel(void *stream, const unsigned char *rgb, int height, int width, const int *table, int num_segments,
                                  int image_index, unsigned char *out_2ch, int *counts, uint64_t *status)
{
    UPS_REQUIRE(rgb && out_2ch && status && ((table && counts) || num_segments == 0), "pan_relabel: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "pan_relabel: bad image size %d x %d", height, width);
    UPS_REQUIRE(num_segments >= 0 && num_segments <= PF_MAX_SEGMENTS, "pan_relabel: %d segments outside 0..%d", num_segments, PF_MAX_SEGMENTS);
    UPS_REQUIRE(image_index >= 0 && image_index < (1 << 24), "pan_relabel: image index %d outside 0..2^24-1", image_index);
    UPS_REQUIRE(((uintptr_t)status & 7) == 0, "pan_relabel: status not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int n = num_segments;
    const long npix = (long)height * width;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const bool use_lds = n <= PF_RELABEL_LDS;
    const bool vec = (((uintptr_t)rgb | (uintptr_t)out_2ch) & 15) == 0;
    hipLaunchKernelGGL(pan_relabel_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), use_lds ? (size_t)n * 3 * sizeof(int) : 0, st,
                       rgb, out_2ch, npix, vec, table, n, use_lds, image_index, counts, (unsigned long long *)status);
    UPS_CHECK_LAUNCH("pan_relabel_kernel");
    if (n > 0) {
        hipLaunchKernelGGL(pan_relabel_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, table, n, image_index, counts,
                           (unsigned long long *)status);
        UPS_CHECK_LAUNCH("pan_relabel_check_kernel");
    }
    return 0;
}
