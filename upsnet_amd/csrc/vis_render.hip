// vis_render.hip -- detection visualisations on the device: what the reference's vis_all_mask draws over the photograph
// (upsnet/dataset/base_dataset.py:826-896, cityscapes.py:236-345: box outline, name.score label, half-transparent mask with a white
// contour), stated as an integer drawing rule of this project instead of matplotlib's rasteriser.
//
// The rule. Canvas = the image, RGB uint8 [H][W][3]. blend(dst, src, a/b) = (dst * (b - a) + src * a + b / 2) / b per channel, integer
// division. The detections come in drawing order. With bx0 = floor(x1), by0 = floor(y1), bx1 = floor(x2), by1 = floor(y2) (each pair
// ordered so that bx0 <= bx1, by0 <= by1; a coordinate beyond +-65536, twice the largest image side, is taken as +-65536, a NaN as
// -65536: none of that moves a visible pixel):
//   1. for every detection in order:
//      a. box outline: green (0,128,0) at 1/2 on the pixels whose Chebyshev distance to the one-pixel rectangle border through the
//         corners is <= 1, i.e. inside [bx0-1, bx1+1] x [by0-1, by1+1] and not inside [bx0+2, bx1-2] x [by0+2, by1-2];
//      b. mask fill: the detection's colour at 1/2 on every mask pixel;
//      c. contour: white at 1/2, on top of b, on every mask pixel with one of its four neighbours outside the mask (a neighbour
//         outside the image is outside the mask);
//   2. then for every detection in order its label of L bytes: the text box is columns bx0 .. bx0 + 12 L - 1, rows by0 - 17 .. by0 - 2
//      (its bottom-left pixel is (bx0, by0 - 2)); green at 2/5 over the whole box, then the glyph dots white and opaque. Character i
//      owns the 12 columns from bx0 + 12 i; its glyph is a 6 x 8 cell (5 x 7 dots, the last column and the last row empty) drawn at
//      scale 2, cell row 0 at the top. Bytes outside 32..126 draw as '?'.
// Everything is clipped to the image. No floating point after the floor.
//
// Launches per image (all on `stream`, nothing synchronised, nothing allocated):
//   ups_zero_async      the bitmaps of this call (fill.hip)
//   vis_prep_kernel     per detection a record: integer box, colour, label length, an empty mask extent
//   vis_bits_kernel     one thread per run of the column-major run lists: sets the run's bits in the detection's bitmap (one bit per
//                       pixel, column-major as the runs are, every column padded to whole 32-bit words so that a column's word k holds
//                       rows 32 k .. 32 k + 31) and widens the detection's extent (integer atomic min / max: a conservative box)
//   vis_compose_kernel  one workgroup per 64 x 32 tile: the 256 threads test one detection each against the tile and compact, in
//                       order, the list of detections whose ring or mask extent meets it and the list of those whose text box does
//                       (ballot + prefix counts, in LDS, with the records). Then every thread owns 4 consecutive pixels of two rows:
//                       it loads their 12 bytes (three dwords where the address allows), walks the first list (ring test; mask: the
//                       column words of its 6 columns give the pixel's bit and its four neighbours), then the second (text box,
//                       glyph dot), and stores the 12 bytes once. No atomics on the canvas: the result is the same on every run.
// Every index a kernel forms is clamped to its array whatever the run lists hold: a malformed list draws a wrong picture, no more.
//
// Limits, refused with an error code: 1 <= H, W <= 32768, H * W <= 2^28, 0 <= n <= 256 detections, labels of at most 32 bytes.
// Workspace: upsnet_vis_workspace_bytes(n, H, W) bytes, 4-byte aligned, NO zeroing asked of the caller (a call zeroes what it reads).
#include <string.h>

#include "common.h"
#include "upsnet_hip.h"
#include "vis_font.h"

#define VIS_MAX_DETS 256
#define VIS_MAX_LABEL 32
#define VIS_MAX_SIDE 32768
#define VIS_MAX_PIXELS (1L << 28)
#define VIS_COORD_LIMIT 65536
#define VIS_REC 12          // ints per record: bx0 by0 bx1 by1 | mx0 my0 mx1 my1 (mask extent, inclusive) | colour | label bytes | 0 0
#define VIS_TW 64
#define VIS_TH 32
#define VIS_PX 4            // pixels per thread and row
#define VIS_CELL_W 12       // a character at scale 2
#define VIS_CELL_H 16
#define VIS_INT_MAX 0x7fffffff

static const unsigned char h_vis_font[][8] = {VIS_FONT_ROWS};
__device__ static const unsigned char d_vis_font[][8] = {VIS_FONT_ROWS};
static_assert(sizeof(h_vis_font) == 95 * 8, "the font has one cell per printable ASCII character");

__device__ static inline int vis_coord(const float v)
{
    float f = floorf(v);
    if (!(f >= -(float)VIS_COORD_LIMIT)) f = -(float)VIS_COORD_LIMIT;   // (also a NaN)
    if (f > (float)VIS_COORD_LIMIT) f = (float)VIS_COORD_LIMIT;
    return (int)f;
}

__global__ void __launch_bounds__(VIS_MAX_DETS)
vis_prep_kernel(const float *__restrict__ boxes, const unsigned char *__restrict__ colours, const int *__restrict__ label_len, const int n,
                int *__restrict__ rec)
{
    const int d = threadIdx.x;
    if (d >= n) return;
    const int x1 = vis_coord(boxes[4 * d]), y1 = vis_coord(boxes[4 * d + 1]), x2 = vis_coord(boxes[4 * d + 2]), y2 = vis_coord(boxes[4 * d + 3]);
    int *r = rec + d * VIS_REC;
    r[0] = min(x1, x2);
    r[1] = min(y1, y2);
    r[2] = max(x1, x2);
    r[3] = max(y1, y2);
    r[4] = VIS_INT_MAX;
    r[5] = VIS_INT_MAX;
    r[6] = -1;
    r[7] = -1;
    r[8] = (int)colours[3 * d] | (int)colours[3 * d + 1] << 8 | (int)colours[3 * d + 2] << 16;
    r[9] = min(max(label_len[d], 0), VIS_MAX_LABEL);
    r[10] = 0;
    r[11] = 0;
}

// rows y0 .. y1 - 1 of one column whose first word is `col`
__device__ static inline void vis_set_bits(unsigned *__restrict__ col, const int y0, const int y1)
{
    const int w0 = y0 >> 5, w1 = (y1 - 1) >> 5;
    const unsigned m0 = ~0u << (y0 & 31), m1 = ~0u >> (31 - ((y1 - 1) & 31));
    if (w0 == w1) {
        atomicOr(col + w0, m0 & m1);
    } else {
        atomicOr(col + w0, m0);
        for (int w = w0 + 1; w < w1; ++w) col[w] = ~0u;   // (a word one run covers whole is no other run's)
        atomicOr(col + w1, m1);
    }
}

__global__ void __launch_bounds__(256)
vis_bits_kernel(const int *__restrict__ trans, const int *__restrict__ trans_off, const int n, const int num_trans, const int H, const int W,
                const int P, unsigned *__restrict__ bits, int *__restrict__ rec)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_trans) return;
    int lo = 0, hi = n - 1;   // the last d with trans_off[d] <= i
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (trans_off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    const int d = lo, first = trans_off[d], last = min(trans_off[d + 1], num_trans);
    if (i < first || i >= last || ((i - first) & 1)) return;   // a run starts at every even position of its list
    const int hw = H * W;
    int s = min(max(trans[i], 0), hw);
    const int e = i + 1 < last ? min(max(trans[i + 1], 0), hw) : hw;
    if (e <= s) return;
    unsigned *bm = bits + (size_t)d * W * P;
    int *r = rec + d * VIS_REC;
    const int xa = s / H, xb = (e - 1) / H;
    atomicMin(r + 4, xa);
    atomicMax(r + 6, xb);
    atomicMin(r + 5, xa == xb ? s - xa * H : 0);
    atomicMax(r + 7, xa == xb ? e - 1 - xa * H : H - 1);
    for (int x = xa; x <= xb; ++x) {
        const int y0 = x == xa ? s - xa * H : 0, y1 = x == xb ? e - xb * H : H;
        vis_set_bits(bm + (size_t)x * P, y0, y1);
    }
}

__device__ static inline unsigned vis_half(const unsigned dst, const unsigned src) { return (dst + src + 1u) >> 1; }

struct VisPx {
    unsigned c[3];
};

__device__ static inline void vis_blend_half(VisPx &p, const unsigned r, const unsigned g, const unsigned b)
{
    p.c[0] = vis_half(p.c[0], r);
    p.c[1] = vis_half(p.c[1], g);
    p.c[2] = vis_half(p.c[2], b);
}

__global__ void __launch_bounds__(256)
vis_compose_kernel(const unsigned char *__restrict__ image, unsigned char *__restrict__ out, const int H, const int W, const int P, const int n,
                   const int *__restrict__ rec, const unsigned *__restrict__ bits, const unsigned char *__restrict__ labels)
{
    __shared__ int s_rec[VIS_MAX_DETS][VIS_REC];
    __shared__ unsigned char s_patch[VIS_MAX_DETS], s_text[VIS_MAX_DETS];
    __shared__ int s_cnt[2][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx0 = blockIdx.x * VIS_TW, ty0 = blockIdx.y * VIS_TH;
    const int tx1 = min(tx0 + VIS_TW, W) - 1, ty1 = min(ty0 + VIS_TH, H) - 1;

    // ---- the tile's two ordered lists
    bool patch = false, text = false;
    if (t < n) {
        int r[VIS_REC];
#pragma unroll
        for (int j = 0; j < VIS_REC; ++j) r[j] = rec[t * VIS_REC + j];
        const bool ring = r[0] - 1 <= tx1 && r[2] + 1 >= tx0 && r[1] - 1 <= ty1 && r[3] + 1 >= ty0;
        const bool mask = r[4] <= tx1 && r[6] >= tx0 && r[5] <= ty1 && r[7] >= ty0;
        patch = ring || mask;
        text = r[9] > 0 && r[0] <= tx1 && r[0] + VIS_CELL_W * r[9] - 1 >= tx0 && r[1] - (VIS_CELL_H + 1) <= ty1 && r[1] - 2 >= ty0;
        if (patch || text) {
#pragma unroll
            for (int j = 0; j < VIS_REC; ++j) s_rec[t][j] = r[j];
        }
    }
    const unsigned long long bp = __ballot(patch), bt = __ballot(text);
    if (lane == 0) {
        s_cnt[0][wave] = __popcll(bp);
        s_cnt[1][wave] = __popcll(bt);
    }
    __syncthreads();
    int base_p = 0, base_t = 0, n_patch = 0, n_text = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (w < wave) {
            base_p += s_cnt[0][w];
            base_t += s_cnt[1][w];
        }
        n_patch += s_cnt[0][w];
        n_text += s_cnt[1][w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    if (patch) s_patch[base_p + __popcll(bp & below)] = (unsigned char)t;
    if (text) s_text[base_t + __popcll(bt & below)] = (unsigned char)t;
    __syncthreads();

    // ---- the pixels: 4 consecutive ones of rows ty0 + (t >> 4) and ty0 + (t >> 4) + 16
    const int x0 = tx0 + VIS_PX * (t & 15);
    if (x0 >= W) return;
    const int npx = min(VIS_PX, W - x0);
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int y = ty0 + (t >> 4) + 16 * half;
        if (y >= H) return;
        const size_t at = ((size_t)y * W + x0) * 3;
        const bool vec = npx == VIS_PX && (((uintptr_t)(image + at) | (uintptr_t)(out + at)) & 3) == 0;
        unsigned w[3] = {0u, 0u, 0u};
        if (vec) {
            const unsigned *src = (const unsigned *)(image + at);
            w[0] = src[0];
            w[1] = src[1];
            w[2] = src[2];
        } else {
            for (int j = 0; j < 3 * npx; ++j) w[j >> 2] |= (unsigned)image[at + j] << (8 * (j & 3));
        }
        VisPx px[VIS_PX];
#pragma unroll
        for (int i = 0; i < VIS_PX; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) px[i].c[c] = (w[(3 * i + c) >> 2] >> (8 * ((3 * i + c) & 3))) & 255u;

        const int k = y >> 5, b = y & 31;
        for (int e = 0; e < n_patch; ++e) {
            const int d = s_patch[e];
            const int *r = s_rec[d];
            const int bx0 = r[0], by0 = r[1], bx1 = r[2], by1 = r[3];
            if (y >= by0 - 1 && y <= by1 + 1 && x0 + VIS_PX - 1 >= bx0 - 1 && x0 <= bx1 + 1) {
                const bool yin = y >= by0 + 2 && y <= by1 - 2;
#pragma unroll
                for (int i = 0; i < VIS_PX; ++i) {
                    const int x = x0 + i;
                    if (x >= bx0 - 1 && x <= bx1 + 1 && !(yin && x >= bx0 + 2 && x <= bx1 - 2)) vis_blend_half(px[i], 0u, 128u, 0u);
                }
            }
            if (y >= r[5] && y <= r[7] && x0 + VIS_PX - 1 >= r[4] && x0 <= r[6]) {
                const unsigned *bm = bits + (size_t)d * W * P;
                unsigned mid[VIS_PX + 2];
#pragma unroll
                for (int j = 0; j < VIS_PX + 2; ++j) {
                    const int xx = x0 - 1 + j;
                    mid[j] = xx >= 0 && xx < W ? bm[(size_t)xx * P + k] : 0u;
                }
                const unsigned cr = (unsigned)r[8] & 255u, cg = (unsigned)r[8] >> 8 & 255u, cb = (unsigned)r[8] >> 16 & 255u;
#pragma unroll
                for (int i = 0; i < VIS_PX; ++i) {
                    const unsigned m = mid[i + 1];
                    if (!(m >> b & 1u)) continue;        // (a column beyond the image reads as 0, and is not stored)
                    const size_t cw = (size_t)(x0 + i) * P + k;
                    const unsigned up = b > 0 ? m >> (b - 1) & 1u : (k > 0 ? bm[cw - 1] >> 31 : 0u);
                    const unsigned dn = b < 31 ? m >> (b + 1) & 1u : (k + 1 < P ? bm[cw + 1] & 1u : 0u);   // (rows past H are never set)
                    const unsigned all4 = up & dn & (mid[i] >> b) & (mid[i + 2] >> b) & 1u;
                    vis_blend_half(px[i], cr, cg, cb);
                    if (!all4) vis_blend_half(px[i], 255u, 255u, 255u);
                }
            }
        }
        for (int e = 0; e < n_text; ++e) {
            const int d = s_text[e];
            const int *r = s_rec[d];
            const int lx0 = r[0], ly0 = r[1] - (VIS_CELL_H + 1), len = r[9];
            const int v = y - ly0;
            if (v < 0 || v >= VIS_CELL_H || x0 + VIS_PX - 1 < lx0 || x0 > lx0 + VIS_CELL_W * len - 1) continue;
#pragma unroll
            for (int i = 0; i < VIS_PX; ++i) {
                const int u = x0 + i - lx0;
                if (u < 0 || u >= VIS_CELL_W * len) continue;
                const int ci = u / VIS_CELL_W, col = (u - ci * VIS_CELL_W) >> 1;
                unsigned ch = labels[d * VIS_MAX_LABEL + ci];
                if (ch < 32u || ch > 126u) ch = '?';
                const bool dot = col < 5 && (d_vis_font[ch - 32u][v >> 1] >> (4 - col) & 1u);
#pragma unroll
                for (int c = 0; c < 3; ++c) px[i].c[c] = dot ? 255u : (px[i].c[c] * 3u + (c == 1 ? 256u : 0u) + 2u) / 5u;
            }
        }

        w[0] = w[1] = w[2] = 0u;
#pragma unroll
        for (int i = 0; i < VIS_PX; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) w[(3 * i + c) >> 2] |= px[i].c[c] << (8 * ((3 * i + c) & 3));
        if (vec) {
            unsigned *dst = (unsigned *)(out + at);
            dst[0] = w[0];
            dst[1] = w[1];
            dst[2] = w[2];
        } else {
            for (int j = 0; j < 3 * npx; ++j) out[at + j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
}

static bool vis_size_ok(int n, int height, int width)
{
    return n >= 0 && n <= VIS_MAX_DETS && height >= 1 && width >= 1 && height <= VIS_MAX_SIDE && width <= VIS_MAX_SIDE &&
           (long)height * width <= VIS_MAX_PIXELS;
}

extern "C" int upsnet_vis_max_detections(void) { return VIS_MAX_DETS; }
extern "C" int upsnet_vis_max_label(void) { return VIS_MAX_LABEL; }

extern "C" size_t upsnet_vis_workspace_bytes(int num_dets, int height, int width)
{
    if (!vis_size_ok(num_dets, height, width)) return 0;
    return ((size_t)VIS_MAX_DETS * VIS_REC + (size_t)num_dets * width * ((height + 31) / 32)) * sizeof(int);
}

extern "C" int upsnet_vis_font(unsigned char *cells)
{
    UPS_REQUIRE(cells != nullptr, "vis_font: null pointer");
    memcpy(cells, h_vis_font, sizeof(h_vis_font));
    return 0;
}

extern "C" int upsnet_vis_render(void *stream, const unsigned char *image, int height, int width, int num_dets, const float *boxes,
                                 const unsigned char *colours, const unsigned char *labels, const int *label_len, const int *trans,
                                 const int *trans_off, int num_trans, void *workspace, unsigned char *out)
{
    UPS_REQUIRE(image && out && workspace, "vis_render: null pointer");
    UPS_REQUIRE(num_dets >= 0 && num_dets <= VIS_MAX_DETS, "vis_render: %d detections outside 0..%d", num_dets, VIS_MAX_DETS);
    UPS_REQUIRE(vis_size_ok(num_dets, height, width), "vis_render: image of %d x %d: sides in 1..%d, at most 2^28 pixels", height, width,
                VIS_MAX_SIDE);
    UPS_REQUIRE(num_dets == 0 || (boxes && colours && labels && label_len && trans_off), "vis_render: null pointer");
    UPS_REQUIRE(num_trans >= 0 && (num_trans == 0 || (trans && num_dets > 0)), "vis_render: %d run boundaries without a list", num_trans);
    UPS_REQUIRE(((uintptr_t)workspace & 3) == 0, "vis_render: workspace not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int P = (height + 31) / 32;
    int *rec = (int *)workspace;
    unsigned *bits = (unsigned *)(rec + VIS_MAX_DETS * VIS_REC);
    if (num_dets > 0) {
        if (ups_zero_async(bits, (size_t)num_dets * width * P * sizeof(int), st)) return 1;
        hipLaunchKernelGGL(vis_prep_kernel, dim3(1), dim3(VIS_MAX_DETS), 0, st, boxes, colours, label_len, num_dets, rec);
        UPS_CHECK_LAUNCH("vis_prep_kernel");
    }
    if (num_trans > 0) {
        hipLaunchKernelGGL(vis_bits_kernel, dim3((unsigned)((num_trans + 255) / 256)), dim3(256), 0, st, trans, trans_off, num_dets, num_trans,
                           height, width, P, bits, rec);
        UPS_CHECK_LAUNCH("vis_bits_kernel");
    }
    hipLaunchKernelGGL(vis_compose_kernel, dim3((unsigned)((width + VIS_TW - 1) / VIS_TW), (unsigned)((height + VIS_TH - 1) / VIS_TH)), dim3(256),
                       0, st, image, out, height, width, P, num_dets, rec, bits, labels);
    UPS_CHECK_LAUNCH("vis_compose_kernel");
    return 0;
}
