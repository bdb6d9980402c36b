// pq_boundary.hip -- Boundary PQ (Cheng et al., Boundary IoU, CVPR 2021) on the device: PQ with every segment pair scored by
// min(mask IoU, boundary IoU). The rule is this project's restatement; tests/boundary_pq_ref.py states it in numpy.
//
// Boundary bit of a pixel of a label map: NOT interior, where interior = the (2d+1) x (2d+1) window centred on the pixel lies inside the
// image and holds the pixel's own label throughout. For every label s, boundary & (label == s) is mask_to_boundary(label == s) of
// DESIGN 4.17, so ONE pass over the label map serves all its segments. The window test is separable and walks no window:
//   pb_row_kernel  one wave per 256 pixels of a row, lanes along x: "a run of equal labels starts here" as one ballot per 64 pixels;
//                  the last start at or before a lane and the first start after it are a count of leading / trailing zeros of the
//                  masked ballot, carried across the wave's four chunks, and across the seam by a look-back / look-ahead of at most
//                  d + 1 pixels that stops at the first start found. rowok = x - last >= d and next - x > d. Written per pixel: rowok and
//                  "same label as the pixel above", two bits per map, one workspace byte for both maps.
//   pb_col_kernel  lanes along x, one thread per column of a slab of max(32, d) rows, ONE sweep down: the run length of rows with rowok
//                  and the label of the row above, saturated at 2d+1; the pixel d rows up is interior iff the run is saturated. The sweep
//                  runs from d rows above its slab to d rows below it (2d extra rows), so it costs at most three times the slab
//                  whatever d.
// When 2d+1 exceeds the height or the width every pixel is boundary and a fill replaces both passes. Labels: GT the 24-bit PNG id, pred
// cat << 8 | inst with every cat == 255 pixel one VOID label. Bit 0 = GT boundary, bit 1 = pred boundary; a map that is not given
// leaves its bit 0.
//
// Counts: pqb_hist_kernel is pq_hist_kernel reading the bit map as well (the pair walk of pan_pixels.h with its third stream: runs
// of equal (pred key, GT id, bits), the same LDS hash) into a SECOND count area that follows the first, so a cell index addresses both:
//   area_bp [key] | void_b [key] | inter_b [row][inst] | area_bg [row]
// pqb_match_kernel is pq_match_kernel with iou = min(iou_m, iou_b), iou_b = inter_b / (area_bp + area_bg - inter_b - void_b) (0 when
// that union is empty); it clears both areas. FP absorption, FN and the summation order are pq_match_kernel's.
#include "common.h"
#include "upsnet_hip.h"
#include "pq_eval.h"

#define PB_K 4                       // 64-pixel chunks per wave in the row pass
#define PB_SEG (UPS_WAVE * PB_K)
#define PB_SLAB_MIN 32               // rows per column-pass slab: max(PB_SLAB_MIN, d)

template <bool PRED>
__device__ static inline unsigned pb_label(const unsigned char *__restrict__ m, const long p)
{
    const unsigned a = m[3 * p], b = m[3 * p + 1];
    if (PRED) return a == 255 ? 0xff00u : a << 8 | b;
    return a | b << 8 | (unsigned)m[3 * p + 2] << 16;
}

// One map, one wave, pixels xs .. xs + PB_SEG - 1 of row y (0 <= xs < W; 2d+1 <= W, so every position below stays under 2^31).
// Returns, for chunk c, bit 2c = rowok and bit 2c+1 = same label as the pixel above, of the lane's pixel xs + 64 c + lane.
template <bool PRED>
__device__ static inline unsigned pb_row_map(const unsigned char *__restrict__ m, const int y, const int xs, const int W, const int d,
                                             const int lane)
{
    const long row = (long)y * W;
    const int xe = xs + PB_SEG;
    // look-back: the last start in [max(0, xs-d-1), xs); none found: any position <= xs - d serves
    int last_c = xs - d - 1;
    if (xs > 0) {
        const int lo = max(0, xs - d - 1);
        for (int hi = xs; hi > lo; hi -= UPS_WAVE) {
            const int p = hi - UPS_WAVE + lane;
            bool s = false;
            if (p >= lo) s = p == 0 || pb_label<PRED>(m, row + p) != pb_label<PRED>(m, row + p - 1);
            const unsigned long long b = __ballot(s);
            if (b) { last_c = hi - 1 - __clzll(b); break; }
        }
    }
    // look-ahead: the first start in [xe, xe+d], the position W counting as one; none found: any position > xe + d - 1 serves
    int next_c = xe + d + 1;
    for (int lo = xe; lo <= xe + d; lo += UPS_WAVE) {
        const int p = lo + lane;
        bool s = false;
        if (p <= xe + d) s = p >= W || pb_label<PRED>(m, row + p) != pb_label<PRED>(m, row + p - 1);
        const unsigned long long b = __ballot(s);
        if (b) { next_c = lo + __builtin_ctzll(b); break; }
    }
    unsigned long long st[PB_K];
    unsigned res = 0;
    unsigned carry = xs > 0 ? pb_label<PRED>(m, row + xs - 1) : 0;
#pragma unroll
    for (int c = 0; c < PB_K; ++c) {
        const int x = xs + UPS_WAVE * c + lane;
        const bool in = x < W;
        const unsigned lab = in ? pb_label<PRED>(m, row + x) : 0;
        unsigned left = __shfl_up(lab, 1);
        if (lane == 0) left = carry;
        carry = __shfl(lab, UPS_WAVE - 1);
        st[c] = __ballot(x == 0 || !in || lab != left);          // W and everything past it start a run
        if (in && y > 0 && pb_label<PRED>(m, row - W + x) == lab) res |= 2u << (2 * c);
    }
#pragma unroll
    for (int c = 0; c < PB_K; ++c) {
        const int base = xs + UPS_WAVE * c;
        const unsigned long long mm = st[c] & (~0ull >> (UPS_WAVE - 1 - lane));
        const int last = mm ? base + 63 - __clzll(mm) : last_c;
        if (base + lane - last >= d) res |= 1u << (2 * c);
        if (st[c]) last_c = base + 63 - __clzll(st[c]);
    }
#pragma unroll
    for (int c = PB_K - 1; c >= 0; --c) {
        const int base = xs + UPS_WAVE * c;
        const unsigned long long mm = lane == UPS_WAVE - 1 ? 0ull : st[c] & (~0ull << (lane + 1));
        const int next = mm ? base + __builtin_ctzll(mm) : next_c;
        if (!(next - (base + lane) > d)) res &= ~(1u << (2 * c));
        if (st[c]) next_c = base + __builtin_ctzll(st[c]);
    }
    return res;
}

// ws byte of a pixel: bit 0 GT rowok, bit 1 pred rowok, bit 2 GT same-as-above, bit 3 pred same-as-above
__global__ void __launch_bounds__(256)
pb_row_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ gt, const int H, const int W, const int d,
              const int segs, unsigned char *__restrict__ ws)
{
    const int lane = threadIdx.x & (UPS_WAVE - 1);
    const long u = (long)blockIdx.x * (256 / UPS_WAVE) + threadIdx.x / UPS_WAVE;   // wave-uniform
    if (u >= (long)H * segs) return;
    const int y = (int)(u / segs), xs = (int)(u % segs) * PB_SEG;
    const unsigned rg = gt ? pb_row_map<false>(gt, y, xs, W, d, lane) : 0;
    const unsigned rp = pred ? pb_row_map<true>(pred, y, xs, W, d, lane) : 0;
#pragma unroll
    for (int c = 0; c < PB_K; ++c) {
        const int x = xs + UPS_WAVE * c + lane;
        if (x < W)
            ws[(long)y * W + x] = (unsigned char)((rg >> (2 * c) & 1) | (rp >> (2 * c) & 1) << 1 | (rg >> (2 * c + 1) & 1) << 2 |
                                                  (rp >> (2 * c + 1) & 1) << 3);
    }
}

__global__ void __launch_bounds__(UPS_WAVE)
pb_col_kernel(const unsigned char *__restrict__ ws, const int H, const int W, const int d, const int slab, const int colgroups,
              const unsigned present, unsigned char *__restrict__ out)
{
    const int x = (int)(blockIdx.x % colgroups) * UPS_WAVE + threadIdx.x;
    if (x >= W) return;
    const int ys = (int)(blockIdx.x / colgroups) * slab, ye = min(H, ys + slab);
    const int sat = 2 * d + 1;
    int ug = 0, up = 0;
#pragma unroll 4
    for (int r = max(0, ys - d); r < ye + d; ++r) {
        if (r < H) {
            const unsigned b = ws[(long)r * W + x];
            ug = (b & 1) ? min(((b & 4) ? ug : 0) + 1, sat) : 0;
            up = (b & 2) ? min(((b & 8) ? up : 0) + 1, sat) : 0;
        } else {
            ug = up = 0;                                         // the window of row r - d leaves the image
        }
        const int y = r - d;
        if (y >= ys) out[(long)y * W + x] = (unsigned char)(((ug < sat ? 1u : 0u) | (up < sat ? 2u : 0u)) & present);
    }
}

__global__ void __launch_bounds__(256)
pb_fill_kernel(unsigned char *__restrict__ out, const long npix, const unsigned char v)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < npix) out[i] = v;
}

// both passes (or the fill) on `st`; arguments already validated
static int pb_launch(hipStream_t st, const int d, const unsigned char *pred, const unsigned char *gt, const int H, const int W,
                     unsigned char *ws, unsigned char *out)
{
    const long npix = (long)H * W;
    const unsigned present = (gt ? 1u : 0u) | (pred ? 2u : 0u);
    if (d > (H - 1) / 2 || d > (W - 1) / 2) {                   // 2d+1 > H or 2d+1 > W: no pixel is interior
        hipLaunchKernelGGL(pb_fill_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, out, npix, (unsigned char)present);
        UPS_CHECK_LAUNCH("pb_fill_kernel");
        return 0;
    }
    const int segs = (W + PB_SEG - 1) / PB_SEG;
    const long waves = (long)H * segs;
    hipLaunchKernelGGL(pb_row_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, pred, gt, H, W, d, segs, ws);
    UPS_CHECK_LAUNCH("pb_row_kernel");
    const int slab = d > PB_SLAB_MIN ? d : PB_SLAB_MIN;
    const int colgroups = (W + UPS_WAVE - 1) / UPS_WAVE;
    const long blocks = (long)colgroups * ((H + slab - 1) / slab);
    hipLaunchKernelGGL(pb_col_kernel, dim3((unsigned)blocks), dim3(UPS_WAVE), 0, st, ws, H, W, d, slab, colgroups, present, out);
    UPS_CHECK_LAUNCH("pb_col_kernel");
    return 0;
}

extern "C" size_t upsnet_pan_boundary_workspace_bytes(int height, int width)
{
    if (height <= 0 || width <= 0 || (long)height * width >= (1L << 31)) return 0;
    return (size_t)height * width;
}

extern "C" int upsnet_pan_boundary_map(void *stream, int dilation, const unsigned char *pred_2ch, const unsigned char *gt_rgb, int height,
                                       int width, void *workspace, unsigned char *out_bits)
{
    UPS_REQUIRE(workspace && out_bits && (pred_2ch || gt_rgb), "pan_boundary_map: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "pan_boundary_map: bad image size %d x %d", height, width);
    UPS_REQUIRE(dilation >= 1, "pan_boundary_map: dilation %d < 1", dilation);
    return pb_launch((hipStream_t)stream, dilation, pred_2ch, gt_rgb, height, width, (unsigned char *)workspace, out_bits);
}

// ---------------------------------------------------------------------------------------------------------------- counts and match
// Second count area, in cells from n1 = 2 * PQ_KEYS + max_gt * 256 (the end of the first):
//   n1 + key: area_bp | n1 + PQ_KEYS + key: void_b | n1 + 2 PQ_KEYS + row * 256 + inst: inter_b | .. + max_gt * 256 + row: area_bg
struct PqbOff {
    unsigned abp, voidb, jointb, abg;
};

static inline PqbOff pqb_off(int max_gt)
{
    PqbOff o;
    o.abp = 2u * PQ_KEYS + (unsigned)max_gt * 256;
    o.voidb = o.abp + PQ_KEYS;
    o.jointb = o.voidb + PQ_KEYS;
    o.abg = o.jointb + (unsigned)max_gt * 256;
    return o;
}

static size_t pqb_cnt_cells(int max_gt) { return (size_t)pqb_off(max_gt).abg + (size_t)((max_gt + 1) & ~1); }   // even: seg stays 8-aligned

// Workspace (bytes): pq_ws with cnt[first area | second area] | (to 16 bytes) | uint8 bits[H*W] | uint8 rows[H*W]. Only the count cells
// and nkeys must be zero between calls.
static size_t pqb_tables_bytes(int max_gt)
{
    const size_t b = pqb_cnt_cells(max_gt) * sizeof(int) + (size_t)max_gt * (sizeof(PqSeg) + sizeof(double)) + (256 + 2 + PQ_KEYS) * sizeof(int);
    return (b + 15) & ~(size_t)15;
}

// one run of `run` pixels with the same pred key, GT id and boundary bits b (bit 0 GT, bit 1 pred)
__device__ static inline void pqb_flush(unsigned *s_key, int *s_val, const PqWs &ws, const int *s_id, const unsigned char *s_cat,
                                        const int n, const PqbOff o, const unsigned pk, const int gid, const unsigned b, const int run)
{
    const unsigned cat = pk >> 8;
    if (cat == 255) return;
    pq_add(s_key, s_val, ws, pk, run);
    if (b & 2) pq_add(s_key, s_val, ws, o.abp + pk, run);
    if (gid == 0) {
        pq_add(s_key, s_val, ws, PQ_VOID_OFF + pk, run);
        if (b & 2) pq_add(s_key, s_val, ws, o.voidb + pk, run);
    } else {
        const int g = pq_find(s_id, n, gid);
        if (g >= 0) {
            if (b & 1) pq_add(s_key, s_val, ws, o.abg + (unsigned)g, run);
            if (s_cat[g] == cat) {
                pq_add(s_key, s_val, ws, PQ_JOINT_OFF + (unsigned)g * 256 + (pk & 255), run);
                if (b == 3) pq_add(s_key, s_val, ws, o.jointb + (unsigned)g * 256 + (pk & 255), run);
            }
        }
    }
}

__global__ void __launch_bounds__(256)
pqb_hist_kernel(const unsigned char *__restrict__ pred, const unsigned char *__restrict__ gt, const unsigned char *__restrict__ bits,
                const long npix, const bool vec, const int n, const PqbOff o, PqWs ws)
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
    if (p0 < npix)   // (bits starts 16-byte aligned in the workspace)
        pan_pair_walk<true>(pred, gt, bits, p0, npix, vec, [&](const unsigned pk, const int gid, const unsigned bb, const int run) {
            pqb_flush(s_key, s_val, ws, s_id, s_cat, n, o, pk, gid, bb, run);
        });
    __syncthreads();
    pan_lds_drain<PQ_HASH_BITS>(s_key, [&](const unsigned k, const int i) { pq_global_add(ws, k, s_val[i]); });
}

// min(mask iou, boundary iou) of GT row g with pred instance inst of its category; both in float64 from integer counts
__device__ static inline double pqb_iou(const int *__restrict__ cnt, const PqbOff o, const long long area_g, const int g, const int cat,
                                        const int inst, const int inter)
{
    const double m = pq_iou(cnt, area_g, cat, inst, inter);
    const int k = cat << 8 | inst;
    const int ib = cnt[o.jointb + (unsigned)g * 256 + inst];
    const long long uni = (long long)cnt[o.abp + k] + cnt[o.abg + g] - ib - cnt[o.voidb + k];
    const double b = uni > 0 ? (double)ib / (double)uni : 0.0;
    return b < m ? b : m;
}

__global__ void __launch_bounds__(PQM_T)
pqb_match_kernel(const int n, const unsigned char *__restrict__ cat_known, const int image_index, const PqbOff o, PqWs ws,
                 int64_t *__restrict__ tp, int64_t *__restrict__ fp, int64_t *__restrict__ fn, double *__restrict__ iou,
                 unsigned long long *__restrict__ status)
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
                    const double v = pqb_iou(cnt, o, s.area, g, s.cat, inst, inter);
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
    // unmatched pred segments: the mask counts decide the absorption, as in pq_match_kernel
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
        if (t == 0) atomicCAS(status, 0ull, (unsigned long long)(image_index + 1) << 8 | (unsigned)s_bad);
    } else if (t < 256) {
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
            } else {   // several matches of one GT segment: instance order
                const long long area_g = ws.seg[g].area;
                for (int inst = 0; inst < 256; ++inst) {
                    const int inter = joint[g * 256 + inst];
                    if (inter > 0) {
                        const double v = pqb_iou(cnt, o, area_g, g, c, inst, inter);
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
    // leave both count areas zeroed for the next image
    for (int i = t; i < nk; i += PQM_T) {
        const int k = ws.keys[i];
        cnt[k] = 0;
        cnt[PQ_VOID_OFF + k] = 0;
        cnt[o.abp + k] = 0;          // boundary cells of a key are only ever counted with its area
        cnt[o.voidb + k] = 0;
    }
    for (int i = t; i < n * 256; i += PQM_T) { cnt[PQ_JOINT_OFF + i] = 0; cnt[o.jointb + i] = 0; }
    for (int i = t; i < n; i += PQM_T) cnt[o.abg + i] = 0;
    if (t == 0) *ws.nkeys = 0;
}

extern "C" size_t upsnet_pq_boundary_workspace_bytes(int max_gt, int height, int width)
{
    if (max_gt < 0 || max_gt > PQ_MAX_GT || height <= 0 || width <= 0 || (long)height * width >= (1L << 31)) return 0;
    const size_t npix = (size_t)height * width;
    return pqb_tables_bytes(max_gt) + ((npix + 15) & ~(size_t)15) + npix;
}

extern "C" int upsnet_pq_boundary_accumulate(void *stream, int dilation, const unsigned char *pred_2ch, const unsigned char *gt_rgb,
                                             int height, int width, const int64_t *segments, int num_segments,
                                             const unsigned char *cat_known, int image_index, int max_gt, void *workspace, int64_t *tp,
                                             int64_t *fp, int64_t *fn, double *iou, uint64_t *status)
{
    UPS_REQUIRE(pred_2ch && gt_rgb && cat_known && workspace && tp && fp && fn && iou && status && (segments || num_segments == 0),
                "pq_boundary_accumulate: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "pq_boundary_accumulate: bad image size %d x %d", height,
                width);
    UPS_REQUIRE(dilation >= 1, "pq_boundary_accumulate: dilation %d < 1", dilation);
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PQ_MAX_GT, "pq_boundary_accumulate: max_gt %d outside 0..%d", max_gt, PQ_MAX_GT);
    UPS_REQUIRE(num_segments >= 0 && num_segments <= max_gt, "pq_boundary_accumulate: %d GT segments, workspace sized for %d", num_segments,
                max_gt);
    UPS_REQUIRE(image_index >= 0 && image_index < (1 << 24), "pq_boundary_accumulate: image index %d outside 0..2^24-1", image_index);
    UPS_REQUIRE(((uintptr_t)workspace & 15) == 0, "pq_boundary_accumulate: workspace not 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const PqWs ws = pq_ws(workspace, pqb_cnt_cells(max_gt), max_gt);
    const PqbOff o = pqb_off(max_gt);
    const int n = num_segments;
    const long npix = (long)height * width;
    unsigned char *bits = (unsigned char *)workspace + pqb_tables_bytes(max_gt);
    unsigned char *rows = bits + ((npix + 15) & ~15L);
    if (pb_launch(st, dilation, pred_2ch, gt_rgb, height, width, rows, bits)) return 1;
    hipLaunchKernelGGL(pq_prep_kernel, dim3(1), dim3(1024), (size_t)n * 2 * sizeof(int), st, segments, n, ws);
    UPS_CHECK_LAUNCH("pq_prep_kernel");
    const bool vec = (((uintptr_t)pred_2ch | (uintptr_t)gt_rgb) & 15) == 0;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const size_t lds = (size_t)PQ_HASH * 2 * sizeof(int) + (size_t)n * (sizeof(int) + 1);
    hipLaunchKernelGGL(pqb_hist_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), lds, st, pred_2ch, gt_rgb, bits, npix, vec, n, o,
                       ws);
    UPS_CHECK_LAUNCH("pqb_hist_kernel");
    hipLaunchKernelGGL(pqb_match_kernel, dim3(1), dim3(PQM_T), (size_t)n * sizeof(int), st, n, cat_known, image_index, o, ws, tp, fp,
                       fn, iou, (unsigned long long *)status);
    UPS_CHECK_LAUNCH("pqb_match_kernel");
    return 0;
}
