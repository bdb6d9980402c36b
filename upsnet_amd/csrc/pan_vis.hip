// pan_vis.hip -- panoptic predictions as pictures, on the device: the vis_panoptic branch of the reference's _converter_2ch_single_core
// (upsnet/dataset/base_dataset.py:463-511: every segment in its category colour, white contours around the thing instances) and the
// same map over the photograph, stated as an integer drawing rule of this project instead of cv2.findContours
// and PIL's two-pixel line.
//
// The rule. pred_2ch uint8 [H][W][3]: channel 0 category (255 = VOID), channel 1 instance; key(p) = ch0 << 8 | ch1. edge(p), for a
// non-VOID pixel: one of its four neighbours has another key or lies outside the image. blend(dst, src, a/b) =
// (dst * (b - a) + src * a + b / 2) / b per channel, integer division (section 4.13's).
//   flat     1. the pixel's CATEGORY colour from the table; VOID and a category that is not in the table are (0,0,0);
//            2. pixel (y, x) is white if one of (y, x), (y, x-1), (y-1, x), (y-1, x-1) lies inside the image and is an edge pixel of a
//               segment with isthing and ch1 != 0 (the contour, widened by one pixel to the right and down).
//   overlay  1. the image pixel; 2. non-VOID: blend(., the segment's colour of upsnet_pan_format's id map, 1/2); 3. edge(p):
//            blend(., white, 1/2) on top, stuff included; 4. after all pixels' steps 1-3 the labels in ascending key: the segments of
//            area >= label_min_area, at most the first 256 of them. Text = the category's name of L bytes (bytes outside 32..126 draw
//            as '?') in the font of vis_font.h at scale 2 (12 x 16 pixels per character); anchor = the integer centroid
//            cx = floor(sum x / area), cy = floor(sum y / area) (64-bit sums); left = cx - 6 L, top = cy - 8, then
//            left = max(min(left, W - 12 L), 0), top = max(min(top, H - 16), 0); black at 2/5 over the box, then the glyph dots white and
//            opaque. Everything is clipped to the image.
// No floating point anywhere; every output byte is stored exactly once; two runs give the same bytes.
//
// Launches per image (all on `stream`, nothing synchronised, nothing allocated); flat is the compose launch alone:
//   pan_moment_kernel   the pixel pass of pan_pixels.h with the row walk, like pan_format.hip's pan_seg_kernel (a run ends with its
//                       key or its row); a run of l pixels from column x0 of row y adds l x0 + l (l - 1) / 2 to its
//                       key's sum of x and l y to its sum of y, in an LDS table per workgroup that falls back to the global 64-bit
//                       atomics when it is full around a slot (a pixel-noise map stays exact); then one pair of global atomics per
//                       distinct key and workgroup.
//   pan_label_kernel    one workgroup: walks the segment table upsnet_pan_format has just written (ascending key), compacts the
//                       segments of area >= label_min_area in order (ballot + prefix counts) into at most 256 label records (text box,
//                       category, length), writes the two counts, and clears every moment cell it read: the workspace is zero again.
//   pan_compose_kernel  one workgroup per 64 x 32 tile. The threads stage the tile's keys with their halo (two pixels up and to the
//                       left, one down and to the right) in LDS and compact, in order, the label records whose box meets the tile.
//                       Then every thread owns 4 consecutive pixels of two rows: it loads their bytes of the image and of the id map
//                       (three dwords each where the address allows), applies the rule, and stores the 12 bytes once.
// Every index a kernel forms is clamped to its array whatever the segment table holds: a malformed table draws a wrong picture, no more.
#include "common.h"
#include "upsnet_hip.h"
#include "vis_font.h"
#include "pan_pixels.h"

#define PV_FLAT 0                 // `mode` of the entry point
#define PV_OVERLAY 1
#define PV_KEYS 65536
#define PV_MAX_SEGMENTS 65280     // rows of upsnet_pan_format's table
#define PV_HEAD 8                 // its ints before the first row
#define PV_ROW 8                  // its ints per row: key, area, ...
#define PV_MAX_LABELS 256
#define PV_MAX_NAME 32
#define PV_MAX_SIDE 32768
#define PV_MAX_PIXELS (1L << 28)
#define PV_HASH_BITS 10           // the moment pass's LDS table: 1024 keys per workgroup, two 64-bit planes
#define PV_HASH (1 << PV_HASH_BITS)
#define PV_TW 64
#define PV_TH 32
#define PV_PX 4                   // pixels per thread and row
#define PV_LW (PV_TW + 3)         // the staged keys: two columns / rows before the tile, one after it
#define PV_LH (PV_TH + 3)
#define PV_OUTSIDE 0x10000u       // "key" of a position outside the image: differs from every key
#define PV_CELL_W 12              // a character at scale 2
#define PV_CELL_H 16
#define PV_LT 1024                // threads of the label kernel

__device__ static const unsigned char d_pv_font[][8] = {VIS_FONT_ROWS};

typedef unsigned long long pv_u64;

// Workspace: sum of x [PV_KEYS] | sum of y [PV_KEYS] (64-bit, zero between calls) | label records int4 [PV_MAX_LABELS] (left, top,
// category, bytes; written before they are read)
struct PvWs {
    pv_u64 *sx, *sy;
    int4 *rec;
};

static PvWs pv_ws(void *base)
{
    PvWs w;
    w.sx = (pv_u64 *)base;
    w.sy = w.sx + PV_KEYS;
    w.rec = (int4 *)(w.sy + PV_KEYS);
    return w;
}

// one run of `run` pixels of one key on row y from column x0
__device__ static inline void pv_flush(unsigned *s_key, pv_u64 *s_sum, const PvWs &ws, const unsigned key, const int run, const int x0, const int y)
{
    if ((key >> 8) == 255) return;   // VOID, whatever its instance
    const pv_u64 mx = (pv_u64)(run * x0 + run * (run - 1) / 2), my = (pv_u64)(run * y);
    const bool held = pan_lds_claim<PV_HASH_BITS>(s_key, key, [&](const unsigned slot) {
        atomicAdd(&s_sum[slot], mx);
        atomicAdd(&s_sum[PV_HASH + slot], my);
    });
    if (!held) {
        atomicAdd(&ws.sx[key], mx);   // LDS table full around this slot (noise-like maps)
        atomicAdd(&ws.sy[key], my);
    }
}

__global__ void __launch_bounds__(256)
pan_moment_kernel(const unsigned char *__restrict__ pred, const long npix, const int width, const bool vec, PvWs ws)
{
    __shared__ unsigned s_key[PV_HASH];
    __shared__ pv_u64 s_sum[2 * PV_HASH];
    pan_lds_clear<PV_HASH_BITS>(s_key, s_sum, 2);
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 < npix)
        pan_row_walk(pred, p0, npix, width, vec, [&](const unsigned key, const int run, const int x0, const int y) {
            pv_flush(s_key, s_sum, ws, key, run, x0, y);
        });
    __syncthreads();
    pan_lds_drain<PV_HASH_BITS>(s_key, [&](const unsigned k, const int i) {
        atomicAdd(&ws.sx[k], s_sum[i]);
        atomicAdd(&ws.sy[k], s_sum[PV_HASH + i]);
    });
}

// table: upsnet_pan_format's (rows in ascending key). info[0] = segments of area >= min_area, info[1] = labels recorded.
__global__ void __launch_bounds__(PV_LT)
pan_label_kernel(const int *__restrict__ table, const int *__restrict__ name_len, const int H, const int W, const int min_area, PvWs ws,
                 int *__restrict__ info)
{
    __shared__ int s_cnt[PV_LT / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = min(max(table[0], 0), PV_MAX_SEGMENTS);
    int base = 0;
    for (int start = 0; start < n; start += PV_LT) {
        const int i = start + t;
        bool q = false;
        int key = 0, area = 0;
        pv_u64 sx = 0, sy = 0;
        if (i < n) {
            const int *row = table + PV_HEAD + (size_t)i * PV_ROW;
            key = row[0] & (PV_KEYS - 1);
            area = row[1];
            sx = ws.sx[key];
            sy = ws.sy[key];
            ws.sx[key] = 0;   // the workspace is zero again for the next image
            ws.sy[key] = 0;
            q = area > 0 && area >= min_area;
        }
        const pv_u64 b = __ballot(q);
        if (lane == 0) s_cnt[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < PV_LT / 64; ++w) {
            if (w < wave) before += s_cnt[w];
            total += s_cnt[w];
        }
        const int pos = base + before + __popcll(b & ((1ull << lane) - 1ull));
        if (q && pos < PV_MAX_LABELS) {
            const int cat = key >> 8;
            const int len = min(max(name_len[cat], 0), PV_MAX_NAME);
            const int cx = (int)min(sx / (pv_u64)area, (pv_u64)(W - 1)), cy = (int)min(sy / (pv_u64)area, (pv_u64)(H - 1));
            const int left = max(min(cx - (PV_CELL_W / 2) * len, W - PV_CELL_W * len), 0);
            const int top = max(min(cy - PV_CELL_H / 2, H - PV_CELL_H), 0);
            ws.rec[pos] = make_int4(left, top, cat, len);
        }
        base += total;
        __syncthreads();
    }
    if (t == 0) {
        info[0] = base;
        info[1] = min(base, PV_MAX_LABELS);
    }
}

__device__ static inline unsigned pv_half(const unsigned dst, const unsigned src) { return (dst + src + 1u) >> 1; }

// is the staged position (ly, lx) a contour pixel: an edge pixel of a thing segment with an instance number
__device__ static inline bool pv_contour(const unsigned *s_key, const int *s_cat, const int ly, const int lx)
{
    const int at = (ly + 2) * PV_LW + lx + 2;
    const unsigned k = s_key[at];
    if (k >= PV_OUTSIDE || (k >> 8) == 255u || (k & 255u) == 0u) return false;
    const int info = s_cat[k >> 8];
    if (info < 0 || !(info >> 24 & 1)) return false;
    return s_key[at - PV_LW] != k || s_key[at + PV_LW] != k || s_key[at - 1] != k || s_key[at + 1] != k;
}

__global__ void __launch_bounds__(256)
pan_compose_kernel(const bool overlay, const unsigned char *__restrict__ pred, const unsigned char *__restrict__ id_rgb,
                   const unsigned char *__restrict__ image, unsigned char *__restrict__ out, const int H, const int W,
                   const int *__restrict__ cat_table, const unsigned char *__restrict__ names, const int4 *__restrict__ rec,
                   int *__restrict__ info)
{
    __shared__ unsigned s_key[PV_LH * PV_LW];
    __shared__ int s_cat[256];
    __shared__ int4 s_rec[PV_MAX_LABELS];
    __shared__ unsigned char s_list[PV_MAX_LABELS];
    __shared__ int s_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int tx0 = blockIdx.x * PV_TW, ty0 = blockIdx.y * PV_TH;
    const int tx1 = min(tx0 + PV_TW, W) - 1, ty1 = min(ty0 + PV_TH, H) - 1;
    const int x0 = tx0 + PV_PX * (t & 15);
    const int npx = min(PV_PX, W - x0);   // (<= 0: the thread owns no pixel of the image)

    // ---- the tile's keys: the thread's own pixels, then the halo
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int ly = (t >> 4) + 16 * half, y = ty0 + ly;
        unsigned k[PV_PX] = {PV_OUTSIDE, PV_OUTSIDE, PV_OUTSIDE, PV_OUTSIDE};
        if (y < H && npx > 0) {
            const size_t at = ((size_t)y * W + x0) * 3;
            unsigned w[3] = {0u, 0u, 0u};
            if (npx == PV_PX && ((uintptr_t)(pred + at) & 3) == 0) {
                const unsigned *src = (const unsigned *)(pred + at);
                w[0] = src[0];
                w[1] = src[1];
                w[2] = src[2];
            } else {
                for (int j = 0; j < 3 * npx; ++j) w[j >> 2] |= (unsigned)pred[at + j] << (8 * (j & 3));
            }
#pragma unroll
            for (int i = 0; i < PV_PX; ++i)
                if (i < npx) k[i] = pan_byte(w, 3 * i) << 8 | pan_byte(w, 3 * i + 1);
        }
#pragma unroll
        for (int i = 0; i < PV_PX; ++i) s_key[(ly + 2) * PV_LW + PV_PX * (t & 15) + i + 2] = k[i];
    }
    for (int i = t; i < 3 * PV_LW + 3 * PV_TH; i += 256) {
        int ly, lx;
        if (i < 2 * PV_LW) {                    // the two rows above, corners included
            ly = i / PV_LW - 2;
            lx = i % PV_LW - 2;
        } else if (i < 3 * PV_LW) {             // the row below
            ly = PV_TH;
            lx = i - 2 * PV_LW - 2;
        } else if (i < 3 * PV_LW + 2 * PV_TH) { // the two columns to the left
            ly = (i - 3 * PV_LW) >> 1;
            lx = ((i - 3 * PV_LW) & 1) - 2;
        } else {                                // the column to the right
            ly = i - 3 * PV_LW - 2 * PV_TH;
            lx = PV_TW;
        }
        const int gy = ty0 + ly, gx = tx0 + lx;
        unsigned k = PV_OUTSIDE;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t at = ((size_t)gy * W + gx) * 3;
            k = (unsigned)pred[at] << 8 | (unsigned)pred[at + 1];
        }
        s_key[(ly + 2) * PV_LW + lx + 2] = k;
    }

    // ---- flat: the category table; overlay: the ordered list of the labels whose box meets the tile
    int n_list = 0;
    if (!overlay) {
        s_cat[t] = cat_table[t];
        if (blockIdx.x == 0 && blockIdx.y == 0 && t < 2) info[t] = 0;
        __syncthreads();
    } else {
        const int n = min(max(info[1], 0), PV_MAX_LABELS);
        bool text = false;
        if (t < n) {
            const int4 r = rec[t];
            text = r.w > 0 && r.x <= tx1 && r.x + PV_CELL_W * r.w - 1 >= tx0 && r.y <= ty1 && r.y + PV_CELL_H - 1 >= ty0;
            if (text) s_rec[t] = r;
        }
        const pv_u64 bt = __ballot(text);
        if (lane == 0) s_cnt[wave] = __popcll(bt);
        __syncthreads();
        int before = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) before += s_cnt[w];
            n_list += s_cnt[w];
        }
        if (text) s_list[before + __popcll(bt & ((1ull << lane) - 1ull))] = (unsigned char)t;
        __syncthreads();
    }

    // ---- the pixels: 4 consecutive ones of rows ty0 + (t >> 4) and ty0 + (t >> 4) + 16
    if (npx <= 0) return;
    const int lx0 = PV_PX * (t & 15);
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        const int ly = (t >> 4) + 16 * half, y = ty0 + ly;
        if (y >= H) return;
        const size_t at = ((size_t)y * W + x0) * 3;
        const unsigned *krow = s_key + (ly + 2) * PV_LW + lx0 + 2;
        unsigned px[PV_PX][3];
        bool vec;
        if (overlay) {
            vec = npx == PV_PX && (((uintptr_t)(image + at) | (uintptr_t)(id_rgb + at) | (uintptr_t)(out + at)) & 3) == 0;
            unsigned w[3] = {0u, 0u, 0u}, c[3] = {0u, 0u, 0u};
            if (vec) {
                const unsigned *src = (const unsigned *)(image + at), *col = (const unsigned *)(id_rgb + at);
                w[0] = src[0]; w[1] = src[1]; w[2] = src[2];
                c[0] = col[0]; c[1] = col[1]; c[2] = col[2];
            } else {
                for (int j = 0; j < 3 * npx; ++j) {
                    w[j >> 2] |= (unsigned)image[at + j] << (8 * (j & 3));
                    c[j >> 2] |= (unsigned)id_rgb[at + j] << (8 * (j & 3));
                }
            }
#pragma unroll
            for (int i = 0; i < PV_PX; ++i) {
                const unsigned k = krow[i];
                const bool seg = k < PV_OUTSIDE && (k >> 8) != 255u;
                const bool edge = seg && (krow[i - PV_LW] != k || krow[i + PV_LW] != k || krow[i - 1] != k || krow[i + 1] != k);
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    unsigned v = pan_byte(w, 3 * i + ch);
                    if (seg) v = pv_half(v, pan_byte(c, 3 * i + ch));
                    if (edge) v = pv_half(v, 255u);
                    px[i][ch] = v;
                }
            }
            for (int e = 0; e < n_list; ++e) {
                const int4 r = s_rec[s_list[e]];
                const int v = y - r.y;
                if (v < 0 || v >= PV_CELL_H || x0 + PV_PX - 1 < r.x || x0 > r.x + PV_CELL_W * r.w - 1) continue;
#pragma unroll
                for (int i = 0; i < PV_PX; ++i) {
                    const int u = x0 + i - r.x;
                    if (u < 0 || u >= PV_CELL_W * r.w) continue;
                    const int ci = min(u / PV_CELL_W, PV_MAX_NAME - 1), col = (u - ci * PV_CELL_W) >> 1;
                    unsigned chr = names[(r.z & 255) * PV_MAX_NAME + ci];
                    if (chr < 32u || chr > 126u) chr = '?';
                    const bool dot = col < 5 && (d_pv_font[chr - 32u][v >> 1] >> (4 - col) & 1u);
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) px[i][ch] = dot ? 255u : (px[i][ch] * 3u + 2u) / 5u;
                }
            }
        } else {
            vec = npx == PV_PX && ((uintptr_t)(out + at) & 3) == 0;
            bool cont[2][PV_PX + 1];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < PV_PX + 1; ++j) cont[r][j] = pv_contour(s_key, s_cat, ly - 1 + r, lx0 - 1 + j);
#pragma unroll
            for (int i = 0; i < PV_PX; ++i) {
                const unsigned k = krow[i];
                unsigned colour = 0u;
                if (k < PV_OUTSIDE && (k >> 8) != 255u) {
                    const int ci = s_cat[k >> 8];
                    if (ci >= 0) colour = (unsigned)ci & 0xffffffu;
                }
                if (cont[0][i] || cont[0][i + 1] || cont[1][i] || cont[1][i + 1]) colour = 0xffffffu;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[i][ch] = colour >> (8 * ch) & 255u;
            }
        }

        unsigned w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < PV_PX; ++i)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) w[(3 * i + ch) >> 2] |= px[i][ch] << (8 * ((3 * i + ch) & 3));
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

extern "C" size_t upsnet_pan_vis_workspace_bytes(void) { return (size_t)2 * PV_KEYS * sizeof(pv_u64) + (size_t)PV_MAX_LABELS * sizeof(int4); }

extern "C" size_t upsnet_pan_vis_workspace_zeroed_bytes(void) { return (size_t)2 * PV_KEYS * sizeof(pv_u64); }

extern "C" int upsnet_pan_vis_max_labels(void) { return PV_MAX_LABELS; }

extern "C" int upsnet_pan_vis(void *stream, int mode, const unsigned char *pred_2ch, const unsigned char *id_rgb, const int *seg_table,
                              const unsigned char *image, int height, int width, const int *cat_table, const unsigned char *names,
                              const int *name_len, int label_min_area, void *workspace, unsigned char *out, int *info)
{
    UPS_REQUIRE(mode == PV_FLAT || mode == PV_OVERLAY, "pan_vis: mode %d is neither flat (%d) nor overlay (%d)", mode,
                PV_FLAT, PV_OVERLAY);
    const bool overlay = mode == PV_OVERLAY;
    UPS_REQUIRE(pred_2ch && cat_table && workspace && out && info, "pan_vis: null pointer");
    UPS_REQUIRE(!overlay || (id_rgb && seg_table && image && names && name_len), "pan_vis: null pointer (overlay)");
    UPS_REQUIRE(height >= 1 && width >= 1 && height <= PV_MAX_SIDE && width <= PV_MAX_SIDE && (long)height * width <= PV_MAX_PIXELS,
                "pan_vis: image of %d x %d: sides in 1..%d, at most 2^28 pixels", height, width, PV_MAX_SIDE);
    UPS_REQUIRE(label_min_area >= 0, "pan_vis: label_min_area %d is negative", label_min_area);
    UPS_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)info & 3) == 0 && ((uintptr_t)seg_table & 3) == 0,
                "pan_vis: workspace not 16-byte aligned, or info / seg_table not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const PvWs ws = pv_ws(workspace);
    if (overlay) {
        const long npix = (long)height * width;
        const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
        hipLaunchKernelGGL(pan_moment_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, pred_2ch, npix, width,
                           ((uintptr_t)pred_2ch & 15) == 0, ws);
        UPS_CHECK_LAUNCH("pan_moment_kernel");
        hipLaunchKernelGGL(pan_label_kernel, dim3(1), dim3(PV_LT), 0, st, seg_table, name_len, height, width, label_min_area, ws, info);
        UPS_CHECK_LAUNCH("pan_label_kernel");
    }
    hipLaunchKernelGGL(pan_compose_kernel, dim3((unsigned)((width + PV_TW - 1) / PV_TW), (unsigned)((height + PV_TH - 1) / PV_TH)), dim3(256), 0,
                       st, overlay, pred_2ch, id_rgb, image, out, height, width, cat_table, names, (const int4 *)ws.rec, info);
    UPS_CHECK_LAUNCH("pan_compose_kernel");
    return 0;
}
