// gt_prepare.hip -- one Cityscapes gtFine_instanceIds map -> every file content the dataset classes derive from it:
// the labelTrainIds map, the panoptic PNG content with its segment table (the devkit's createTrainIdLabelImgs / createPanopticImgs),
// and per instance the run-length transitions of its mask (the exact form of Detectron's convert_cityscapes_to_coco annotation).
// The devkit and Detectron are not part of the reference tree: the rules are restated here and in dataset/prepare.py.
//
// Raw value v: label v when v < 1000, label v / 1000 with an instance number when v >= 1000. The three label tables are arguments
// (train id with 255 = ignored, hasInstances, thing row 0..7 or -1): no Cityscapes constant lives in this file. The tables have 256
// entries, so a value encodes a label only in 0..255 or 1000..65535; any other (negative, 256..999, beyond 16 bits) raises
// GP_FLAG_RANGE, counts as ignored and never indexes a table.
//   segment  = a distinct v whose label is not ignored; iscrowd = (v < 1000 and the label has instances);
//   instance = a distinct v >= 1000 whose label has a thing row.
// Integers only, six launches, a workspace that every call leaves zeroed:
//   gp_seg_kernel     one pass over the pixels, 16 per thread: train-id map, panoptic RGB (v as R + 256 G + 65536 B, ignored -> 0),
//                     the labelIds cross-check, and the area / bbox of every segment: runs of one value on one row go into the LDS
//                     table and the bbox payload of pan_pixels.h (a full LDS table falls back to the global atomics). The walk is
//                     the kernel's own: its per-pixel outputs are woven into it.
//   gp_table_kernel   one workgroup: compacts the non-empty values in ascending v into the segment table and the instance list,
//                     and zeroes every workspace cell it read. More segments than the capacity: flag, rows past it are not written.
//   gp_trans_kernel   one workgroup per instance, over its bounding box only: tiles of up to 64 columns are read along the rows
//                     (coalesced) into an LDS bit matrix by wave ballots, then walked column by column; every thread takes 8
//                     consecutive cells, a workgroup scan orders the change positions x * H + y. Run twice: counting, then -- after
//                     gp_scan_kernel turned the counts into trans_off and checked the capacity -- filling. The same code counts
//                     and fills, so a list can never outgrow its place. No atomics: ascending by construction.
#include "common.h"
#include "upsnet_hip.h"
#include "pan_pixels.h"

#define GP_KEYS 65536             // raw values of a 16-bit PNG
#define GP_HASH_BITS 10           // the pixel pass's LDS table: 1024 values per workgroup, five planes
#define GP_HASH (1 << GP_HASH_BITS)
#define GP_ROW 9                  // v, label, train id, iscrowd, area, x_min, y_min, x_max, y_max
#define GP_STATUS 8               // segments | instances | transitions | flags | labelIds mismatches | 0 0 0
#define GP_FLAG_SEGMENTS 1
#define GP_FLAG_TRANSITIONS 2
#define GP_FLAG_RANGE 4
#define GP_INST 5                 // workspace row of an instance: v, x_min, y_min, x_max, y_max
#define GP_TT 256                 // threads of the transition kernel
#define GP_CELLS 8                // consecutive cells per thread and round
#define GP_BIT_WORDS 4096         // 64-bit words of the LDS bit matrix: 2^18 cells
#define GP_MAX_SIDE 32768         // 8 columns of the tallest box still fit the bit matrix
#define GP_TRANS_GRID 1024

struct GpWs {
    int *area, *nxmin, *nymin, *xmax, *ymax;   // [GP_KEYS] each, zero between calls: the five planes of pan_pixels.h's bbox payload
    int *inst;                                 // [seg_cap][GP_INST]
    int *cnt;                                  // [seg_cap] transitions per instance
};

static GpWs gp_ws(void *base, const int seg_cap)
{
    GpWs w;
    int *p = (int *)base;
    w.area = p;
    w.nxmin = p + GP_KEYS;
    w.nymin = p + 2 * GP_KEYS;
    w.xmax = p + 3 * GP_KEYS;
    w.ymax = p + 4 * GP_KEYS;
    w.inst = p + 5 * GP_KEYS;
    w.cnt = w.inst + (size_t)seg_cap * GP_INST;
    return w;
}

// label of a raw value (0..255), or -1 for a value that encodes none
__device__ static inline int gp_label(const int raw)
{
    if (raw < 0 || raw >= GP_KEYS) return -1;
    if (raw < 256) return raw;
    return raw < 1000 ? -1 : raw / 1000;   // at most 65
}

// label info in LDS: train id | hasInstances << 8 | (thing row + 1) << 16
__device__ static inline void gp_load_labels(int *s_lab, const int *__restrict__ train_id, const int *__restrict__ has_inst,
                                             const int *__restrict__ thing_row)
{
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        s_lab[i] = (train_id[i] & 255) | (has_inst[i] != 0) << 8 | ((thing_row[i] + 1) & 255) << 16;
}

__global__ void __launch_bounds__(256)
gp_seg_kernel(const int *__restrict__ ids, const unsigned char *__restrict__ label_ids, const long npix, const int width, const bool vec,
              const int *__restrict__ train_id, const int *__restrict__ has_inst, const int *__restrict__ thing_row, GpWs ws,
              unsigned char *__restrict__ train_map, unsigned char *__restrict__ rgb, int *__restrict__ status)
{
    __shared__ unsigned s_key[GP_HASH];
    __shared__ int s_val[5 * GP_HASH];
    __shared__ int s_lab[256];
    pan_lds_clear<GP_HASH_BITS>(s_key, s_val, 5);
    gp_load_labels(s_lab, train_id, has_inst, thing_row);
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 < npix) {
        const bool whole = vec && p0 + PAN_RUN <= npix;
        const int cnt = (int)(npix - p0 < PAN_RUN ? npix - p0 : PAN_RUN);
        int v[PAN_RUN];
        unsigned lab[4] = {0, 0, 0, 0};
        if (whole) {
            const int4 *src = (const int4 *)(ids + p0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int4 a = src[j];
                v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
            }
            if (label_ids) {
                const uint4 a = *(const uint4 *)(label_ids + p0);
                lab[0] = a.x; lab[1] = a.y; lab[2] = a.z; lab[3] = a.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < PAN_RUN; ++i) {
                v[i] = i < cnt ? ids[p0 + i] : 0;
                if (label_ids && i < cnt) lab[i >> 2] |= (unsigned)label_ids[p0 + i] << (8 * (i & 3));
            }
        }
        unsigned tr[4] = {0, 0, 0, 0}, o[12];
#pragma unroll
        for (int j = 0; j < 12; ++j) o[j] = 0;
        int x = (int)(p0 % width), y = (int)(p0 / width);
        unsigned pk = 0;
        int run = 0, x0 = 0, ry = 0, mismatch = 0;
        bool range = false, live = false;
#pragma unroll
        for (int i = 0; i < PAN_RUN; ++i) {
            if (i < cnt) {
                const int raw = v[i];
                const int label = gp_label(raw);
                const bool ok = label >= 0;
                range |= !ok;
                const unsigned tid = ok ? (unsigned)s_lab[label] & 255u : 255u;
                if (label_ids) mismatch += !ok || (lab[i >> 2] >> (8 * (i & 3)) & 255u) != (unsigned)label;
                tr[i >> 2] |= tid << (8 * (i & 3));
                const unsigned c = tid == 255u ? 0u : (unsigned)raw;
#pragma unroll
                for (int b = 0; b < 3; ++b) o[(3 * i + b) >> 2] |= (c >> (8 * b) & 255u) << (8 * ((3 * i + b) & 3));
                const unsigned k = (unsigned)raw;
                if (run == 0 || k != pk || x == 0) {   // a run shares its value and its row
                    if (run && live) pan_box_add<GP_HASH_BITS>(s_key, s_val, ws.area, pk, run, x0, ry);
                    pk = k;
                    run = 0;
                    x0 = x;
                    ry = y;
                    live = tid != 255u;
                }
                ++run;
                if (++x == width) { x = 0; ++y; }
            }
        }
        if (run && live) pan_box_add<GP_HASH_BITS>(s_key, s_val, ws.area, pk, run, x0, ry);
        if (whole) {
            *(uint4 *)(train_map + p0) = make_uint4(tr[0], tr[1], tr[2], tr[3]);
            uint4 *dst = (uint4 *)(rgb + 3 * p0);
            dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
            dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
            dst[2] = make_uint4(o[8], o[9], o[10], o[11]);
        } else {
#pragma unroll
            for (int i = 0; i < PAN_RUN; ++i)
                if (i < cnt) {
                    train_map[p0 + i] = (unsigned char)(tr[i >> 2] >> (8 * (i & 3)));
#pragma unroll
                    for (int b = 0; b < 3; ++b) rgb[3 * (p0 + i) + b] = (unsigned char)(o[(3 * i + b) >> 2] >> (8 * ((3 * i + b) & 3)));
                }
        }
        if (mismatch) atomicAdd(&status[4], mismatch);
        if (range) atomicOr(&status[3], GP_FLAG_RANGE);
    }
    __syncthreads();
    pan_box_drain<GP_HASH_BITS>(s_key, s_val, ws.area);
}

#define GPT_T 1024
#define GPT_PER (GP_KEYS / GPT_T)   // 64 consecutive values per thread

// inclusive scan of one int per thread over the GPT_T threads; s_scan int [2][GPT_T]; returns the buffer index of the result
__device__ static inline int gp_block_scan(int (*s_scan)[GPT_T], const int mine)
{
    const int t = threadIdx.x;
    s_scan[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < GPT_T; d <<= 1) {
        s_scan[cur ^ 1][t] = s_scan[cur][t] + (t >= d ? s_scan[cur][t - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    return cur;
}

__global__ void __launch_bounds__(GPT_T)
gp_table_kernel(const int *__restrict__ train_id, const int *__restrict__ has_inst, const int *__restrict__ thing_row, GpWs ws,
                const int seg_cap, int *__restrict__ table, int *__restrict__ status)
{
    __shared__ int s_scan[2][GPT_T];
    __shared__ int s_lab[256];
    const int t = threadIdx.x;
    gp_load_labels(s_lab, train_id, has_inst, thing_row);
    __syncthreads();
    int segs = 0, insts = 0;
    for (int j = 0; j < GPT_PER; ++j) {
        const int v = t * GPT_PER + j;
        const int label = gp_label(v);
        if (ws.area[v] != 0 && label >= 0) {   // (the pixel pass leaves the cells of values without a label empty)
            ++segs;
            insts += v >= 1000 && (s_lab[label] >> 16) != 0;
        }
    }
    int cur = gp_block_scan(s_scan, segs);
    const int n_seg = s_scan[cur][GPT_T - 1];
    int pos = s_scan[cur][t] - segs;
    __syncthreads();
    cur = gp_block_scan(s_scan, insts);
    const int n_inst = s_scan[cur][GPT_T - 1];
    int ipos = s_scan[cur][t] - insts;
    for (int j = 0; j < GPT_PER; ++j) {
        const int v = t * GPT_PER + j, a = ws.area[v];
        if (a == 0) continue;
        const int label = gp_label(v);
        const int x_min = PAN_INV - ws.nxmin[v], y_min = PAN_INV - ws.nymin[v], x_max = ws.xmax[v], y_max = ws.ymax[v];
        ws.area[v] = 0;   // the workspace is zero again for the next image, overflow or not
        ws.nxmin[v] = 0;
        ws.nymin[v] = 0;
        ws.xmax[v] = 0;
        ws.ymax[v] = 0;
        if (label < 0) continue;
        const int info = s_lab[label];
        if (pos < seg_cap) {
            int *row = table + (size_t)pos * GP_ROW;
            row[0] = v;
            row[1] = label;
            row[2] = info & 255;
            row[3] = v < 1000 && (info >> 8 & 1);
            row[4] = a;
            row[5] = x_min;
            row[6] = y_min;
            row[7] = x_max;
            row[8] = y_max;
        }
        ++pos;
        if (v >= 1000 && (info >> 16) != 0) {
            if (ipos < seg_cap) {
                int *row = ws.inst + (size_t)ipos * GP_INST;
                row[0] = v;
                row[1] = x_min;
                row[2] = y_min;
                row[3] = x_max;
                row[4] = y_max;
            }
            ++ipos;
        }
    }
    if (t == 0) {
        status[0] = n_seg;
        status[1] = n_inst;
        if (n_seg > seg_cap) atomicOr(&status[3], GP_FLAG_SEGMENTS);
    }
}

// instances the transition kernels work on: none once the segment table has overflowed
__device__ static inline int gp_live_instances(const int *status) { return (status[3] & GP_FLAG_SEGMENTS) ? 0 : status[1]; }

__device__ static inline int gp_bit(const unsigned long long *s_bits, const int b) { return (int)(s_bits[b >> 6] >> (b & 63) & 1ull); }

// Exclusive offset of `mine` among the GP_TT threads and the workgroup total; s_part int [GP_TT / 64 + 1]
__device__ static inline int gp_offset(int *s_part, const int mine, int *total)
{
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int inc = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    __syncthreads();   // (the previous round's reads of s_part are over)
    if (lane == 63) s_part[wave] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < GP_TT / 64; ++w) {
        const int s = s_part[w];
        before += w < wave ? s : 0;
        all += s;
    }
    *total = all;
    return before + inc - mine;
}

// FILL false: cnt[j] = number of change positions of instance j. FILL true: they are written, ascending, from trans[trans_off[j]].
// A change position is a p = x * H + y < H * W at which (ids == v) differs from its value at p - 1 (0 before p = 0): the convention of
// dataset/rle.py::counts_from_transitions. Only the instance's box is read: above and below it the mask is 0, so each column of the
// box closes with a virtual cell of 0 below it -- unless the box spans the whole height, where the cell before (x, 0) is (x - 1, H - 1).
template <bool FILL>
__global__ void __launch_bounds__(GP_TT)
gp_trans_kernel(const int *__restrict__ ids, const int height, const int width, GpWs ws, const int *__restrict__ status,
                const int *__restrict__ trans_off, const int trans_cap, int *__restrict__ trans)
{
    __shared__ unsigned long long s_bits[GP_BIT_WORDS];
    __shared__ int s_part[GP_TT / 64 + 1];
    const int n = gp_live_instances(status);
    if (FILL && (status[3] & GP_FLAG_TRANSITIONS)) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long npix = (long)height * width;
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const int *row = ws.inst + (size_t)j * GP_INST;
        const int v = row[0], x_min = row[1], y_min = row[2], x_max = row[3], y_max = row[4];
        const int h = y_max - y_min + 1;
        const bool full = h == height;
        const int hh = full ? h : h + 1;            // cells walked per column
        int tw_shift = 6;
        while (((long)h << tw_shift) > (long)GP_BIT_WORDS * 64) --tw_shift;   // h <= 32768: at least 8 columns per tile
        const int TW = 1 << tw_shift;
        const int words = (int)((((long)h << tw_shift) + 63) >> 6);
        const long out0 = FILL ? (long)trans_off[j] : 0;
        int base = 0, carry = 0;
        for (int x0 = x_min; x0 <= x_max; x0 += TW) {
            const int tw = min(TW, x_max - x0 + 1);
            __syncthreads();                        // (the previous tile's bits are no longer read)
            for (int w = wave; w < words; w += GP_TT / 64) {
                const int b = w * 64 + lane, r = b >> tw_shift, c = b & (TW - 1);
                const bool in = r < h && c < tw;
                const bool on = in && ids[(long)(y_min + r) * width + x0 + c] == v;
                const unsigned long long m = __ballot(on);
                if (lane == 0) s_bits[w] = m;
            }
            __syncthreads();
            const long cells = (long)tw * hh;
            for (long e0 = 0; e0 < cells; e0 += GP_TT * GP_CELLS) {
                const long e = e0 + (long)t * GP_CELLS;
                int c = (int)(e / hh), r = (int)(e % hh);
                int pos[GP_CELLS];
                unsigned hit = 0;
#pragma unroll
                for (int i = 0; i < GP_CELLS; ++i) {
                    if (e + i < cells) {
                        const int cur = r < h ? gp_bit(s_bits, (r << tw_shift) + c) : 0;
                        int prev;
                        if (r > 0) prev = gp_bit(s_bits, ((r - 1) << tw_shift) + c);
                        else prev = full ? (c > 0 ? gp_bit(s_bits, ((h - 1) << tw_shift) + c - 1) : carry) : 0;
                        const long p = (long)(x0 + c) * height + y_min + r;
                        pos[i] = (int)p;
                        if (cur != prev && p < npix) hit |= 1u << i;
                        if (++r == hh) { r = 0; ++c; }
                    }
                }
                int total;
                const int ofs = gp_offset(s_part, __popc(hit), &total);
                if (FILL) {
                    long at = out0 + base + ofs;
#pragma unroll
                    for (int i = 0; i < GP_CELLS; ++i)
                        if (hit >> i & 1) {
                            if (at < trans_cap) trans[at] = pos[i];
                            ++at;
                        }
                }
                base += total;
            }
            carry = gp_bit(s_bits, ((h - 1) << tw_shift) + tw - 1);   // (x, H - 1) of the tile's last column, for a full-height box
        }
        // a full-height box whose last column ends set: the mask changes at the top of the next column, if there is one
        if (full && carry && (long)(x_max + 1) * height < npix) {
            if (FILL && t == 0 && out0 + base < trans_cap) trans[out0 + base] = (x_max + 1) * height;
            ++base;
        }
        if (!FILL && t == 0) ws.cnt[j] = base;
    }
}

// trans_off[0 .. n] = exclusive sums of cnt[0 .. n); status[2] = their total; more than trans_cap: flag, nothing is filled
__global__ void __launch_bounds__(GPT_T)
gp_scan_kernel(GpWs ws, const int trans_cap, int *__restrict__ trans_off, int *__restrict__ status)
{
    __shared__ int s_scan[2][GPT_T];
    const int t = threadIdx.x;
    const int n = gp_live_instances(status);
    const int per = (n + GPT_T - 1) / GPT_T;
    long sum = 0;
    for (int i = t * per; i < min(n, (t + 1) * per); ++i) sum += ws.cnt[i];
    // (a total beyond 2^31 cannot occur: every position holds at most two changes and H * W < 2^30 is required)
    const int cur = gp_block_scan(s_scan, (int)sum);
    int run = s_scan[cur][t] - (int)sum;
    for (int i = t * per; i < min(n, (t + 1) * per); ++i) {
        trans_off[i] = run;
        run += ws.cnt[i];
    }
    if (t == GPT_T - 1) {
        const int total = s_scan[cur][GPT_T - 1];
        trans_off[n] = total;
        status[2] = total;
        if (total > trans_cap) atomicOr(&status[3], GP_FLAG_TRANSITIONS);
    }
}

extern "C" size_t upsnet_gt_prepare_workspace_bytes(int seg_capacity)
{
    if (seg_capacity < 1 || seg_capacity > GP_KEYS) return 0;
    return ((size_t)5 * GP_KEYS + (size_t)seg_capacity * (GP_INST + 1)) * sizeof(int);
}

extern "C" int upsnet_gt_prepare(void *stream, const int *ids, const unsigned char *label_ids, int height, int width, const int *train_id,
                                 const int *has_instances, const int *thing_row, int seg_capacity, int trans_capacity, void *workspace,
                                 unsigned char *train_map, unsigned char *rgb, int *table, int *trans_off, int *trans, int *status)
{
    UPS_REQUIRE(ids && train_id && has_instances && thing_row && workspace && train_map && rgb && table && trans_off && status,
                "gt_prepare: null pointer");
    UPS_REQUIRE(trans || trans_capacity == 0, "gt_prepare: null transition buffer of capacity %d", trans_capacity);
    UPS_REQUIRE(height > 0 && width > 0 && height <= GP_MAX_SIDE && width <= GP_MAX_SIDE && (long)height * width < (1L << 30),
                "gt_prepare: bad image size %d x %d", height, width);
    UPS_REQUIRE(seg_capacity >= 1 && seg_capacity <= GP_KEYS, "gt_prepare: segment capacity %d outside 1..%d", seg_capacity, GP_KEYS);
    UPS_REQUIRE(trans_capacity >= 0, "gt_prepare: negative transition capacity %d", trans_capacity);
    UPS_REQUIRE((((uintptr_t)workspace | (uintptr_t)ids | (uintptr_t)table | (uintptr_t)trans_off | (uintptr_t)trans | (uintptr_t)status) & 3) == 0,
                "gt_prepare: a 4-byte array is not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const GpWs ws = gp_ws(workspace, seg_capacity);
    const long npix = (long)height * width;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    const bool vec = (((uintptr_t)ids | (uintptr_t)label_ids | (uintptr_t)train_map | (uintptr_t)rgb) & 15) == 0;
    if (ups_zero_async(status, GP_STATUS * sizeof(int), st)) return 1;
    hipLaunchKernelGGL(gp_seg_kernel, dim3(grid), dim3(256), 0, st, ids, label_ids, npix, width, vec, train_id, has_instances, thing_row, ws,
                       train_map, rgb, status);
    UPS_CHECK_LAUNCH("gp_seg_kernel");
    hipLaunchKernelGGL(gp_table_kernel, dim3(1), dim3(GPT_T), 0, st, train_id, has_instances, thing_row, ws, seg_capacity, table, status);
    UPS_CHECK_LAUNCH("gp_table_kernel");
    hipLaunchKernelGGL(gp_trans_kernel<false>, dim3(GP_TRANS_GRID), dim3(GP_TT), 0, st, ids, height, width, ws, status, trans_off,
                       trans_capacity, trans);
    UPS_CHECK_LAUNCH("gp_trans_kernel<count>");
    hipLaunchKernelGGL(gp_scan_kernel, dim3(1), dim3(GPT_T), 0, st, ws, trans_capacity, trans_off, status);
    UPS_CHECK_LAUNCH("gp_scan_kernel");
    hipLaunchKernelGGL(gp_trans_kernel<true>, dim3(GP_TRANS_GRID), dim3(GP_TT), 0, st, ids, height, width, ws, status, trans_off,
                       trans_capacity, trans);
    UPS_CHECK_LAUNCH("gp_trans_kernel<fill>");
    return 0;
}
