// det_eval.hip -- COCO box / mask AP on the device: pycocotools' COCOeval (iouType 'bbox' / 'segm', default Params) restated.
//
// Per image (dataset/coco_eval.py: DetectionEvaluator.add), with no host synchronisation:
//   det_rank_kernel    category row of every detection (class -> row table) and its rank inside (image, row): score descending,
//                      ties in input order (computeIoU's mergesort of -score), ranks >= 100 dropped (maxDets[-1]); writes the
//                      detection's record (score, image, row, rank) and the slot table [row][rank] -> detection
//   det_paste_kernel   segm, model masks: the im_post paste rule (impaste.h) into a column-major bit plane, box region only
//   det_pack_rle_kernel / det_pack_u8_kernel
//                      segm: run-length (transition list) or uint8 masks into full column-major bit planes + pixel counts
//   bnd_erode_kernel   boundary ('boundary' of the Boundary IoU API's COCOeval): mask & ~erode(mask, (2d+1) x (2d+1)) of every det and
//                      GT plane over its rectangle, bit-parallel and separable -- down a column by the nearest zero of the
//                      neighbouring words, across columns by a doubled window in LDS; the IoU is then min(mask IoU, boundary IoU)
//   det_iou_kernel     one workgroup per (row, det slot): IoU against every GT of the row -- bbIou in double for boxes, integer
//                      intersection / union over the det's plane rectangle (__popcll) for masks (rleIou)
//   det_match_kernel   one wavefront per row, one lane per (area range, IoU threshold): evaluateImg's greedy matching; the
//                      matched / ignored bits of each detection go into its record, the non-ignored GT count into npig
// At the end (DetectionEvaluator.accumulate), over all records:
//   count / scan / scatter / order kernels: records bucketed by row, then each record's position in its row's list for
//                      maxDet 1 / 10 / 100 by counting the records before it in (-score, image_id order, rank) -- accumulate's
//                      mergesort over images concatenated in ascending image_id, each truncated to maxDet
//   det_curve_kernel   one workgroup per (row, area, maxDet, threshold): cumulative TP / FP, recall, precision, the reverse max
//                      envelope and the searchsorted of the recall thresholds, in two passes over the list
// Everything compares and divides exactly as the numpy code does (build flag -ffp-contract=off), so precision / recall / scores are
// bit-identical to pycocotools' arrays.
#include <algorithm>

#include "common.h"
#include "impaste.h"
#include "upsnet_hip.h"

#define DE_MAXDET 100   // maxDets[-1]
#define DE_T 10         // len(iouThrs)
#define DE_A 4          // len(areaRng)
#define DE_M 3          // len(maxDets)
#define DE_R 101        // len(recThrs)
#define DE_BT 256

typedef unsigned long long de_u64;

__constant__ static const int de_maxdets[DE_M] = {1, 10, 100};

// ------------------------------------------------------------------------------------------------------------------ per image
__global__ void det_zero_kernel(int *__restrict__ p, const int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0;
}

__global__ void __launch_bounds__(DE_BT)
det_rank_kernel(const int n, const double *__restrict__ score, const int64_t *__restrict__ cls, const int *__restrict__ lut,
                const int lut_n, const int image_index, int *__restrict__ rank_out, int *__restrict__ slot, int *__restrict__ nd,
                int *__restrict__ plane_of, int *__restrict__ nplanes, double *__restrict__ rec_score, int *__restrict__ rec_img, int *__restrict__ rec_rk)
{
    const int i = blockIdx.x * DE_BT + threadIdx.x;
    if (i >= n) return;
    const int64_t c = cls[i];
    const int row = (c >= 0 && c < lut_n) ? lut[c] : -1;
    const double s = score[i];
    int r = -1;
    if (row >= 0) {
        r = 0;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            if (cls[j] != c) continue;   // classes and rows correspond one to one (the host refuses repeated category ids)
            const double sj = score[j];
            r += (sj > s || (sj == s && j < i)) ? 1 : 0;
        }
        if (r >= DE_MAXDET) r = -1;
    }
    rank_out[i] = r;
    rec_score[i] = s;
    rec_img[i] = image_index;
    rec_rk[i] = r >= 0 ? (row << 8 | r) : -1;
    if (r >= 0) {
        slot[row * DE_MAXDET + r] = i;
        atomicMax(&nd[row], r + 1);
    }
    // segm: only the evaluated dets get a mask plane (at most min(n, 100 per row)), numbered by arrival
    if (plane_of) plane_of[i] = r >= 0 ? atomicAdd(nplanes, 1) : -1;
}

// bit planes: plane p at planes + p * W * nw, column x at word x * nw, row y at bit (y & 63) of word y >> 6 (nw = ceil(H / 64));
// rect[p] = (x_0, x_1, w_0, w_1): the columns / words that hold the mask (outside them the plane is not written and reads as 0)
__global__ void __launch_bounds__(DE_BT)
det_paste_kernel(const float *__restrict__ boxes, const float *__restrict__ mask_prob, const int64_t *__restrict__ cls_inds,
                 const int *__restrict__ plane_of, const int num_ch, const int ms, const int H, const int W, de_u64 *__restrict__ planes,
                 int *__restrict__ rect, int *__restrict__ area)
{
    __shared__ float s_pad[IMP_MAXMS * IMP_MAXMS];
    __shared__ int s_area;
    const int d = blockIdx.x, tid = threadIdx.x;
    if (plane_of[d] < 0) {   // not evaluated (category not scored, or rank >= 100): empty, no plane
        if (tid < 4) rect[d * 4 + tid] = 0;
        if (tid == 0) area[d] = 0;
        return;
    }
    const int ps = ms + 2, nw = (H + 63) >> 6;
    imp_load_pad(s_pad, mask_prob, cls_inds, d, num_ch, ms, tid, DE_BT);
    if (tid == 0) s_area = 0;
    const ImpBox b = imp_box(boxes + d * 4, ms, H, W);
    __syncthreads();
    const bool empty = b.x_1 <= b.x_0 || b.y_1 <= b.y_0;
    const int w0 = empty ? 0 : b.y_0 >> 6, w1 = empty ? 0 : ((b.y_1 - 1) >> 6) + 1, nwr = w1 - w0;
    if (tid == 0) {
        rect[d * 4 + 0] = empty ? 0 : b.x_0; rect[d * 4 + 1] = empty ? 0 : b.x_1;
        rect[d * 4 + 2] = w0; rect[d * 4 + 3] = w1;
    }
    if (empty) { if (tid == 0) area[d] = 0; return; }
    de_u64 *plane = planes + (long)plane_of[d] * W * nw;
    const long nwords = (long)(b.x_1 - b.x_0) * nwr;
    int cnt = 0;
    for (long q = tid; q < nwords; q += DE_BT) {
        const int x = b.x_0 + (int)(q / nwr), w = w0 + (int)(q % nwr);
        const int ya = max(w << 6, b.y_0), yb = min((w << 6) + 64, b.y_1);
        de_u64 bits = 0;
        for (int y = ya; y < yb; ++y)
            if (pan_resize_at(s_pad, ps, b.w, b.h, x - b.bx0, y - b.by0) > 0.5f) bits |= 1ull << (y & 63);
        plane[(long)x * nw + w] = bits;
        cnt += __popcll(bits);
    }
    atomicAdd(&s_area, cnt);
    __syncthreads();
    if (tid == 0) area[d] = s_area;
}

// transition lists (column-major positions where the mask value changes, the first one starting a run of ones) -> full planes.
// Mask j: trans[off[j] .. off[j+1]) for mask p = dst[j] (j when dst is null) into plane plane_of[j] (p when plane_of is null; a
// negative entry: not evaluated, left empty); one thread per word (blockIdx.y = mask).
__global__ void __launch_bounds__(DE_BT)
det_pack_rle_kernel(const int *__restrict__ trans, const int64_t *__restrict__ off, const int *__restrict__ dst,
                    const int *__restrict__ plane_of, const int H, const int W, de_u64 *__restrict__ planes, int *__restrict__ rect,
                    int *__restrict__ area)
{
    const int j = blockIdx.y, nw = (H + 63) >> 6;
    const long q = (long)blockIdx.x * DE_BT + threadIdx.x;
    const int *t = trans + off[j];
    const int nt = (int)(off[j + 1] - off[j]);
    const int p = dst ? dst[j] : j;
    const int pl = plane_of ? plane_of[j] : p;
    if (pl < 0) {
        if (blockIdx.x == 0 && threadIdx.x < 4 && rect) rect[p * 4 + threadIdx.x] = 0;
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && rect) {
        // columns holding a set pixel: from the first transition to the last one (an odd count runs to the end of the image)
        rect[p * 4 + 0] = nt ? t[0] / H : 0;
        rect[p * 4 + 1] = nt ? ((nt & 1) ? W : (t[nt - 1] - 1) / H + 1) : 0;
        rect[p * 4 + 2] = 0;
        rect[p * 4 + 3] = nt ? nw : 0;
    }
    if (q >= (long)W * nw) return;
    const int x = (int)(q / nw), w = (int)(q - (long)x * nw);
    const long lo = (long)x * H + (w << 6), hi = (long)x * H + min((w << 6) + 64, H);
    // k = number of transitions <= lo (value at lo = k & 1)
    int a = 0, b = nt;
    while (a < b) { const int m = (a + b) >> 1; if ((long)t[m] <= lo) a = m + 1; else b = m; }
    int k = a;
    de_u64 bits = 0;
    long pos = lo;
    while (pos < hi) {
        const long next = k < nt ? min((long)t[k], hi) : hi;
        if ((k & 1) && next > pos) {
            const int s = (int)(pos - lo), e = (int)(next - lo);
            bits |= (e - s == 64 ? ~0ull : ((1ull << (e - s)) - 1ull)) << s;
        }
        pos = next > pos ? next : pos;
        if (k < nt && (long)t[k] <= pos) ++k;
    }
    planes[(long)pl * W * nw + q] = bits;
    const int c = __popcll(bits);
    if (c) atomicAdd(&area[p], c);
}

// uint8 [H,W] row-major mask (non-zero = set) -> full plane p
__global__ void __launch_bounds__(DE_BT)
det_pack_u8_kernel(const unsigned char *__restrict__ mask, const int p, const int H, const int W, de_u64 *__restrict__ planes,
                   int *__restrict__ area)
{
    const int nw = (H + 63) >> 6;
    const long q = (long)blockIdx.x * DE_BT + threadIdx.x;   // x fastest: neighbouring threads read neighbouring bytes
    if (q >= (long)W * nw) return;
    const int w = (int)(q / W), x = (int)(q - (long)w * W);
    de_u64 bits = 0;
    for (int y = w << 6; y < min((w << 6) + 64, H); ++y)
        if (mask[(long)y * W + x]) bits |= 1ull << (y & 63);
    planes[(long)p * W * nw + (long)x * nw + w] = bits;
    const int c = __popcll(bits);
    if (c) atomicAdd(&area[p], c);
}

// ------------------------------------------------------------------------------------------------------------------ boundary
// mask_to_boundary of the Boundary IoU API: d rounds of a 3x3 erosion of the zero-padded mask = the AND over the (2d+1) x (2d+1)
// window with everything outside the image read as 0; boundary = mask & ~eroded.
#define BND_LDS_WORDS 6144                    // 48 KiB of window words per workgroup
#define BND_ITEMS (BND_LDS_WORDS / DE_BT)     // words a thread holds across one doubling step

__global__ void bnd_full_rect_kernel(int *__restrict__ rect, const int n, const int W, const int nw)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rect[i * 4 + 0] = 0; rect[i * 4 + 1] = W; rect[i * 4 + 2] = 0; rect[i * 4 + 3] = nw;
}

// word w of column `col` (words [w0, w1) of the rectangle; every other word reads as 0) eroded along the column: bit y survives iff
// no zero lies within d rows of it. Inside the word the zeros are smeared d (<= 63) bits both ways; of a neighbouring word only its
// zero nearest to this word matters.
__device__ static inline de_u64 bnd_erode_column_word(const de_u64 *__restrict__ col, const int w, const int w0, const int w1, const int d)
{
    const de_u64 z = ~col[w];
    de_u64 up = z, dn = z;
    const int n = min(d, 63);
    for (int c = 0; c < n;) {
        const int t = min(c + 1, n - c);
        up |= up << t; dn |= dn >> t;
        c += t;
    }
    de_u64 r = up | dn;
    const int q = (d + 63) >> 6;
    for (int j = 1; j <= q && r != ~0ull; ++j) {
        const de_u64 za = w + j < w1 ? ~col[w + j] : ~0ull;   // the word j further down the column: its lowest zero reaches back to row 64j + b - d
        if (za) {
            const int lo = 64 * j + __builtin_ctzll(za) - d;
            if (lo <= 63) r |= lo <= 0 ? ~0ull : ~0ull << lo;
        }
        const de_u64 zb = w - j >= w0 ? ~col[w - j] : ~0ull;  // the word j before: its highest zero reaches on to row -64j + b + d
        if (zb) {
            const int hi = -64 * j + (63 - __builtin_clzll(zb)) + d;
            if (hi >= 0) r |= hi >= 63 ? ~0ull : (2ull << hi) - 1ull;
        }
    }
    return ~r;
}

// Entry e = blockIdx.y: plane plane_of[e] (e when plane_of is null; negative: not evaluated, nothing written) with rectangle rect[e];
// blockIdx.x = (tile of TX columns, slab of WS words) of that rectangle, blocks past it return. The column-eroded words of the
// tile's columns and d more on either side (zero outside the rectangle) go to LDS as [column][word of the slab]; log2 steps of
// P[c] &= P[c + k] leave the AND over p = 2^k columns from c on, and the window of 2d+1 is two of them, at c and at c + 2d+1 - p.
// d < 0: nothing survives the erosion (2d+1 exceeds the image), the boundary is the mask. cnt[e] += the boundary's pixels.
__global__ void __launch_bounds__(DE_BT)
bnd_erode_kernel(const de_u64 *__restrict__ planes, const int *__restrict__ rect, const int *__restrict__ plane_of, const int H, const int W,
                 const int d, const int TX, const int WS, de_u64 *__restrict__ out, int *__restrict__ cnt)
{
    extern __shared__ de_u64 s_win[];
    __shared__ int s_red[DE_BT / UPS_WAVE];
    const int e = blockIdx.y, tid = threadIdx.x, nw = (H + 63) >> 6;
    const int pl = plane_of ? plane_of[e] : e;
    if (pl < 0) return;
    const int x0 = rect[e * 4 + 0], x1 = rect[e * 4 + 1], w0 = rect[e * 4 + 2], w1 = rect[e * 4 + 3];
    const int slabs = (nw + WS - 1) / WS;
    const int xa = x0 + (int)(blockIdx.x / slabs) * TX, wa = w0 + (int)(blockIdx.x % slabs) * WS;
    if (xa >= x1 || wa >= w1) return;
    const int xb = min(xa + TX, x1), ws = min(WS, w1 - wa);
    const de_u64 *plane = planes + (long)pl * W * nw;
    de_u64 *oplane = out + (long)pl * W * nw;
    const int L = 2 * d + 1;
    int p = 1;
    if (d >= 0) {
        const int ca = xa - d, n = (xb - xa + 2 * d) * ws;   // n <= (TX + 2d) * WS <= BND_LDS_WORDS
        for (int q = tid; q < n; q += DE_BT) {
            const int x = ca + q / ws, w = wa + q % ws;
            s_win[q] = (x >= x0 && x < x1) ? bnd_erode_column_word(plane + (long)x * nw, w, w0, w1, d) : 0ull;
        }
        __syncthreads();
        for (; 2 * p <= L; p <<= 1) {
            de_u64 r[BND_ITEMS];
#pragma unroll
            for (int i = 0; i < BND_ITEMS; ++i) {
                const int q = tid + i * DE_BT;
                if (q < n) r[i] = s_win[q] & (q + p * ws < n ? s_win[q + p * ws] : 0ull);
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < BND_ITEMS; ++i) {
                const int q = tid + i * DE_BT;
                if (q < n) s_win[q] = r[i];
            }
            __syncthreads();
        }
    }
    int c = 0;
    const int no = (xb - xa) * ws;
    for (int q = tid; q < no; q += DE_BT) {
        const long o = (long)(xa + q / ws) * nw + wa + q % ws;
        const de_u64 m = plane[o];
        const de_u64 er = d >= 0 ? s_win[q] & s_win[q + (L - p) * ws] : 0ull;
        const de_u64 b = m & ~er;
        oplane[o] = b;
        c += __popcll(b);
    }
    for (int s = UPS_WAVE / 2; s > 0; s >>= 1) c += __shfl_xor(c, s);
    if ((tid & (UPS_WAVE - 1)) == 0) s_red[tid / UPS_WAVE] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int wv = 0; wv < DE_BT / UPS_WAVE; ++wv) t += s_red[wv];
        if (t) atomicAdd(&cnt[e], t);
    }
}

// planes (inside each plane's rectangle, 0 outside it) -> uint8 [n][H][W] masks of 0 / 1; x fastest: neighbouring threads write
// neighbouring bytes
__global__ void __launch_bounds__(DE_BT)
bnd_unpack_u8_kernel(const de_u64 *__restrict__ planes, const int *__restrict__ rect, const int H, const int W, unsigned char *__restrict__ mask)
{
    const int p = blockIdx.y, nw = (H + 63) >> 6;
    const long q = (long)blockIdx.x * DE_BT + threadIdx.x;
    if (q >= (long)W * nw) return;
    const int w = (int)(q / W), x = (int)(q - (long)w * W);
    const bool in = x >= rect[p * 4 + 0] && x < rect[p * 4 + 1] && w >= rect[p * 4 + 2] && w < rect[p * 4 + 3];
    const de_u64 bits = in ? planes[((long)p * W + x) * nw + w] : 0ull;
    unsigned char *o = mask + (long)p * H * W;
    for (int y = w << 6; y < min((w << 6) + 64, H); ++y) o[(long)y * W + x] = (unsigned char)((bits >> (y & 63)) & 1);
}

struct BndTile { int d, TX, WS, grid_x; size_t lds; };

// the tile of bnd_erode_kernel for dilation d on an H x W image; false when the window does not fit the LDS budget
static bool bnd_tile(int H, int W, int d, BndTile *t)
{
    const int nw = (int)(((long)H + 63) / 64);
    if (2L * d + 1 > H || 2L * d + 1 > W) {   // every window leaves the image: nothing survives
        t->d = -1; t->WS = std::min(nw, 16); t->TX = std::min(W, BND_LDS_WORDS / t->WS); t->lds = 0;
    } else {
        if (2L * d + 32 > BND_LDS_WORDS) return false;
        t->d = d;
        t->WS = std::min(nw, BND_LDS_WORDS / (2 * d + 32));
        t->TX = std::min(std::min(W, 256), BND_LDS_WORDS / t->WS - 2 * d);
        t->lds = sizeof(de_u64) * (size_t)(t->TX + 2 * d) * t->WS;
    }
    const long grid = (((long)W + t->TX - 1) / t->TX) * (((long)nw + t->WS - 1) / t->WS);
    if (grid > 0x7fffffffL) return false;
    t->grid_x = (int)grid;
    return true;
}

static int bnd_launch(hipStream_t st, const BndTile &t, const de_u64 *planes, const int *rect, const int *plane_of, int n, int H, int W,
                      de_u64 *out, int *cnt)
{
    UPS_REQUIRE(n <= 65535, "boundary: %d masks in one call (at most 65535)", n);
    UPS_CHECK_HIP(hipMemsetAsync(cnt, 0, sizeof(int) * n, st));
    hipLaunchKernelGGL(bnd_erode_kernel, dim3(t.grid_x, n), dim3(DE_BT), t.lds, st, planes, rect, plane_of, H, W, t.d, t.TX, t.WS, out, cnt);
    UPS_CHECK_LAUNCH("bnd_erode_kernel");
    return 0;
}

// IoU of det slot (row, d) against the row's GTs -> ious[100 * off_k + d * G_k + g]. bbox: bbIou (maskApi.c) on xywh doubles,
// det xywh from xyxy as xyxy_to_xywh does (w = x2 - x1 + 1). segm: rleIou, i / u over pixel counts. With boundary planes (det_bnd
// non-null; the GT ones are written inside gt_rect only) the result is the smaller of the mask's and the boundary's rleIou.
__global__ void __launch_bounds__(DE_BT)
det_iou_kernel(const int segm, const int *__restrict__ rows, const int *__restrict__ slot, const int *__restrict__ nd,
               const double *__restrict__ det_xyxy, const int *__restrict__ det_rect, const int *__restrict__ det_area,
               const int *__restrict__ plane_of, const de_u64 *__restrict__ det_planes, const int *__restrict__ gt_off, const double *__restrict__ gt_box,
               const int *__restrict__ gt_crowd, const de_u64 *__restrict__ gt_planes, const int *__restrict__ gt_area, const int H,
               const int W, double *__restrict__ ious, const de_u64 *__restrict__ det_bnd, const int *__restrict__ det_barea,
               const de_u64 *__restrict__ gt_bnd, const int *__restrict__ gt_barea, const int *__restrict__ gt_rect)
{
    __shared__ int s_red[DE_BT / UPS_WAVE], s_redb[DE_BT / UPS_WAVE];
    const int k = rows[blockIdx.y], d = blockIdx.x, tid = threadIdx.x;
    if (d >= nd[k]) return;
    const int g0 = gt_off[k], G = gt_off[k + 1] - g0;
    const int i = slot[k * DE_MAXDET + d];
    double *out = ious + (long)DE_MAXDET * g0 + (long)d * G;
    if (!segm) {
        const double dx = det_xyxy[i * 4 + 0], dy = det_xyxy[i * 4 + 1];
        const double dw = det_xyxy[i * 4 + 2] - dx + 1.0, dh = det_xyxy[i * 4 + 3] - dy + 1.0;
        const double da = dw * dh;
        for (int g = tid; g < G; g += DE_BT) {
            const double *gb = gt_box + (long)(g0 + g) * 4;
            const double ga = gb[2] * gb[3];
            double o = 0.0;
            const double w = fmin(dw + dx, gb[2] + gb[0]) - fmax(dx, gb[0]);
            if (w > 0) {
                const double h = fmin(dh + dy, gb[3] + gb[1]) - fmax(dy, gb[1]);
                if (h > 0) {
                    const double in = w * h;
                    const double u = gt_crowd[g0 + g] ? da : da + ga - in;
                    o = in / u;
                }
            }
            out[g] = o;
        }
        return;
    }
    const int nw = (H + 63) >> 6;
    const int x0 = det_rect[i * 4 + 0], x1 = det_rect[i * 4 + 1], w0 = det_rect[i * 4 + 2], w1 = det_rect[i * 4 + 3];
    const int nwr = w1 - w0;
    const long nwords = (x1 > x0 && nwr > 0) ? (long)(x1 - x0) * nwr : 0;
    const de_u64 *dp = det_planes + (long)plane_of[i] * W * nw;
    const long da = det_area[i];
    if (!det_bnd) {
        for (int g = 0; g < G; ++g) {
            const de_u64 *gp = gt_planes + (long)(g0 + g) * W * nw;
            int c = 0;
            for (long q = tid; q < nwords; q += DE_BT) {
                const long o = (long)(x0 + (int)(q / nwr)) * nw + w0 + (int)(q % nwr);
                c += __popcll(dp[o] & gp[o]);
            }
            for (int s = UPS_WAVE / 2; s > 0; s >>= 1) c += __shfl_xor(c, s);
            if ((tid & (UPS_WAVE - 1)) == 0) s_red[tid / UPS_WAVE] = c;
            __syncthreads();
            if (tid == 0) {
                long in = 0;
                for (int wv = 0; wv < DE_BT / UPS_WAVE; ++wv) in += s_red[wv];
                const long u = gt_crowd[g0 + g] ? da : da + (long)gt_area[g0 + g] - in;
                out[g] = in == 0 ? 0.0 : (double)in / (double)u;
            }
            __syncthreads();
        }
        return;
    }
    const de_u64 *bp = det_bnd + (long)plane_of[i] * W * nw;
    const long dba = det_barea[i];
    for (int g = 0; g < G; ++g) {
        const de_u64 *gp = gt_planes + (long)(g0 + g) * W * nw, *gbp = gt_bnd + (long)(g0 + g) * W * nw;
        const int *gr = gt_rect + (long)(g0 + g) * 4;
        const int gx0 = gr[0], gx1 = gr[1], gw0 = gr[2], gw1 = gr[3];
        int c = 0, cb = 0;
        for (long q = tid; q < nwords; q += DE_BT) {
            const int x = x0 + (int)(q / nwr), w = w0 + (int)(q % nwr);
            const long o = (long)x * nw + w;
            c += __popcll(dp[o] & gp[o]);
            if (x >= gx0 && x < gx1 && w >= gw0 && w < gw1) cb += __popcll(bp[o] & gbp[o]);
        }
        for (int s = UPS_WAVE / 2; s > 0; s >>= 1) { c += __shfl_xor(c, s); cb += __shfl_xor(cb, s); }
        if ((tid & (UPS_WAVE - 1)) == 0) { s_red[tid / UPS_WAVE] = c; s_redb[tid / UPS_WAVE] = cb; }
        __syncthreads();
        if (tid == 0) {
            long in = 0, inb = 0;
            for (int wv = 0; wv < DE_BT / UPS_WAVE; ++wv) { in += s_red[wv]; inb += s_redb[wv]; }
            const int crowd = gt_crowd[g0 + g];
            const long u = crowd ? da : da + (long)gt_area[g0 + g] - in;
            const long ub = crowd ? dba : dba + (long)gt_barea[g0 + g] - inb;
            const double m = in == 0 ? 0.0 : (double)in / (double)u, b = inb == 0 ? 0.0 : (double)inb / (double)ub;
            out[g] = fmin(m, b);
        }
        __syncthreads();
    }
}

// evaluateImg (maxDet 100) for row blockIdx.x: lane l < A*T takes area range a = l / T and threshold t = l % T. GTs are visited
// non-ignored first, then ignored, each in input order (the stable argsort of _ignore); gtm holds each lane's matched GTs.
__global__ void __launch_bounds__(UPS_WAVE)
det_match_kernel(const int segm, const int *__restrict__ slot, const int *__restrict__ nd, const double *__restrict__ det_xyxy,
                 const int *__restrict__ det_area, const int *__restrict__ gt_off, const double *__restrict__ gt_area,
                 const int *__restrict__ gt_crowd, const double *__restrict__ ious, const double *__restrict__ params,
                 unsigned char *__restrict__ gtm_ws, de_u64 *__restrict__ rec_match, de_u64 *__restrict__ rec_ign,
                 int64_t *__restrict__ npig)
{
    __shared__ unsigned char s_m[DE_MAXDET][DE_A * DE_T], s_ig[DE_MAXDET][DE_A * DE_T];
    const int k = blockIdx.x, l = threadIdx.x;
    const int g0 = gt_off[k], G = gt_off[k + 1] - g0, D = nd[k];
    const bool lane = l < DE_A * DE_T;
    const int a = l / DE_T, t = l - (l / DE_T) * DE_T;
    const double thr = lane ? params[t] : 0.0;
    const double lo = lane ? params[DE_T + 2 * a] : 0.0, hi = lane ? params[DE_T + 2 * a + 1] : 0.0;
    if (lane && t == 0 && G > 0) {
        long c = 0;
        for (int g = 0; g < G; ++g) c += !(gt_crowd[g0 + g] || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi);
        atomicAdd((unsigned long long *)&npig[k * DE_A + a], (unsigned long long)c);
    }
    if (D == 0) return;
    const double *io = ious + (long)DE_MAXDET * g0;
    unsigned char *gtm = gtm_ws + (long)DE_A * DE_T * g0 + (long)l * G;
    if (lane) {
        for (int g = 0; g < G; ++g) gtm[g] = 0;
        for (int d = 0; d < D; ++d) {
            double iou = thr;
            int m = -1, mig = 0;
            for (int pass = 0; pass < 2 && G > 0; ++pass) {
                bool stop = false;
                for (int g = 0; g < G; ++g) {
                    const int crowd = gt_crowd[g0 + g];
                    const int ig = crowd || gt_area[g0 + g] < lo || gt_area[g0 + g] > hi;
                    if (ig != pass) continue;
                    if (gtm[g] && !crowd) continue;
                    if (m > -1 && mig == 0 && ig == 1) { stop = true; break; }
                    const double v = io[(long)d * G + g];
                    if (v < iou) continue;
                    iou = v; m = g; mig = ig;
                }
                if (stop) break;
            }
            const int i = slot[k * DE_MAXDET + d];
            double darea;
            if (segm) darea = (double)det_area[i];
            else {
                const double dw = det_xyxy[i * 4 + 2] - det_xyxy[i * 4 + 0] + 1.0, dh = det_xyxy[i * 4 + 3] - det_xyxy[i * 4 + 1] + 1.0;
                darea = dw * dh;
            }
            if (m > -1) gtm[m] = 1;
            s_m[d][l] = m > -1;
            s_ig[d][l] = m > -1 ? mig : (darea < lo || darea > hi);
        }
    }
    __syncthreads();
    for (int d = l; d < D; d += UPS_WAVE) {
        de_u64 mb = 0, ib = 0;
        for (int q = 0; q < DE_A * DE_T; ++q) {
            mb |= (de_u64)s_m[d][q] << q;
            ib |= (de_u64)s_ig[d][q] << q;
        }
        const int i = slot[k * DE_MAXDET + d];
        rec_match[i] = mb;
        rec_ign[i] = ib;
    }
}

// ------------------------------------------------------------------------------------------------------------------ accumulate
struct DetAccLayout {
    int *cnt, *off, *fill, *total, *bucket, *bkey, *sorted;
    double *bscore;
};

static inline size_t de_align(size_t x) { return (x + 255) & ~(size_t)255; }

static DetAccLayout det_acc_layout(void *ws, long N, int K, size_t *bytes)
{
    DetAccLayout L;
    size_t o = 0;
    const auto at = [ws](size_t off) { return ws ? (char *)ws + off : nullptr; };   // (a size-only call passes no workspace)
    L.cnt = (int *)at(o); o += de_align(sizeof(int) * K * DE_M);
    L.off = (int *)at(o); o += de_align(sizeof(int) * K * DE_M);
    L.fill = (int *)at(o); o += de_align(sizeof(int) * K);
    L.total = (int *)at(o); o += de_align(sizeof(int));
    L.bscore = (double *)at(o); o += de_align(sizeof(double) * N);
    L.bucket = (int *)at(o); o += de_align(sizeof(int) * N);
    L.bkey = (int *)at(o); o += de_align(sizeof(int) * N);
    L.sorted = (int *)at(o); o += de_align(sizeof(int) * N * DE_M);
    if (bytes) *bytes = o;
    return L;
}

__global__ void __launch_bounds__(DE_BT)
det_count_kernel(const long N, const int *__restrict__ rec_rk, int *__restrict__ cnt)
{
    const long i = (long)blockIdx.x * DE_BT + threadIdx.x;
    if (i >= N) return;
    const int rk = rec_rk[i];
    if (rk < 0) return;
    const int row = rk >> 8, r = rk & 255;
    for (int m = 0; m < DE_M; ++m)
        if (r < de_maxdets[m]) atomicAdd(&cnt[row * DE_M + m], 1);
}

// one workgroup: exclusive offsets of each maxDet's lists over the rows (the buckets use the maxDet-100 offsets)
__global__ void __launch_bounds__(DE_BT)
det_scan_kernel(const int K, const int *__restrict__ cnt, int *__restrict__ off, int *__restrict__ fill, int *__restrict__ total)
{
    const int tid = threadIdx.x;
    if (tid < DE_M) {
        int s = 0;
        for (int k = 0; k < K; ++k) { off[k * DE_M + tid] = s; s += cnt[k * DE_M + tid]; }
        if (tid == DE_M - 1) *total = s;
    }
    for (int k = tid; k < K; k += DE_BT) fill[k] = 0;
}

__global__ void __launch_bounds__(DE_BT)
det_scatter_kernel(const long N, const double *__restrict__ rec_score, const int *__restrict__ rec_img, const int *__restrict__ rec_rk,
                   const int *__restrict__ img_ord, const int *__restrict__ off, int *__restrict__ fill, double *__restrict__ bscore,
                   int *__restrict__ bucket, int *__restrict__ bkey)
{
    const long i = (long)blockIdx.x * DE_BT + threadIdx.x;
    if (i >= N) return;
    const int rk = rec_rk[i];
    if (rk < 0) return;
    const int row = rk >> 8;
    const int p = off[row * DE_M + DE_M - 1] + atomicAdd(&fill[row], 1);
    bscore[p] = rec_score[i];
    bucket[p] = (int)i;
    bkey[p] = img_ord[rec_img[i]] << 8 | (rk & 255);   // (image position in ascending image_id, rank): the tie order
}

// position of bucket entry p in its row's list for each maxDet: the entries of the row that precede it in (-score, image, rank)
__global__ void __launch_bounds__(DE_BT)
det_order_kernel(const int K, const int *__restrict__ rec_rk, const int *__restrict__ cnt, const int *__restrict__ off,
                 const int *__restrict__ total, const double *__restrict__ bscore, const int *__restrict__ bucket,
                 const int *__restrict__ bkey, int *__restrict__ sorted, const long N)
{
    const long p = (long)blockIdx.x * DE_BT + threadIdx.x;
    if (p >= *total) return;
    const int i = bucket[p];
    const int row = rec_rk[i] >> 8;
    const int b0 = off[row * DE_M + DE_M - 1], b1 = b0 + cnt[row * DE_M + DE_M - 1];
    const double s = bscore[p];
    const int key = bkey[p], r = key & 255;
    int c[DE_M] = {0, 0, 0};
    for (int q = b0; q < b1; ++q) {
        const double sq = bscore[q];
        const int kq = bkey[q];
        if (sq > s || (sq == s && kq < key)) {
            const int rq = kq & 255;
            for (int m = 0; m < DE_M; ++m) c[m] += rq < de_maxdets[m];
        }
    }
    for (int m = 0; m < DE_M; ++m)
        if (r < de_maxdets[m]) sorted[(long)m * N + off[row * DE_M + m] + c[m]] = i;
}

__device__ static inline int de_block_sum(int v, int *s_red)
{
    for (int s = UPS_WAVE / 2; s > 0; s >>= 1) v += __shfl_xor(v, s);
    __syncthreads();
    if ((threadIdx.x & (UPS_WAVE - 1)) == 0) s_red[threadIdx.x / UPS_WAVE] = v;
    __syncthreads();
    int t = 0;
    for (int w = 0; w < DE_BT / UPS_WAVE; ++w) t += s_red[w];
    return t;
}

// accumulate for (row k, area a, maxDet m, threshold t) = blockIdx.x decomposed; outputs in pycocotools' layouts
// precision / scores [T,R,K,A,M], recall [T,K,A,M].
__global__ void __launch_bounds__(DE_BT)
det_curve_kernel(const int K, const int64_t *__restrict__ npig, const int *__restrict__ cnt, const int *__restrict__ off,
                 const int *__restrict__ sorted, const long N, const double *__restrict__ rec_score, const de_u64 *__restrict__ rec_match,
                 const de_u64 *__restrict__ rec_ign, const double *__restrict__ rec_thrs, double *__restrict__ precision,
                 double *__restrict__ recall, double *__restrict__ scores)
{
    __shared__ int s_red[DE_BT / UPS_WAVE];
    __shared__ int s_tp[DE_BT], s_fp[DE_BT];
    __shared__ double s_env[DE_BT];
    __shared__ double s_thr[DE_R];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int t = b % DE_T; b /= DE_T;
    const int m = b % DE_M; b /= DE_M;
    const int a = b % DE_A; b /= DE_A;
    const int k = b;
    const long KAM = (long)K * DE_A * DE_M, kam = ((long)k * DE_A + a) * DE_M + m;
    const int64_t np = npig[k * DE_A + a];
    if (np == 0) {   // no non-ignored GT (or no evaluated image at all): -1, as pycocotools leaves it
        for (int r = tid; r < DE_R; r += DE_BT) {
            precision[((long)t * DE_R + r) * KAM + kam] = -1.0;
            scores[((long)t * DE_R + r) * KAM + kam] = -1.0;
        }
        if (tid == 0) recall[(long)t * KAM + kam] = -1.0;
        return;
    }
    for (int r = tid; r < DE_R; r += DE_BT) {
        s_thr[r] = rec_thrs[r];
        precision[((long)t * DE_R + r) * KAM + kam] = 0.0;   // recall thresholds past the end of rc stay 0 (the try / except)
        scores[((long)t * DE_R + r) * KAM + kam] = 0.0;
    }
    const int nd = cnt[k * DE_M + m];
    const int *list = sorted + (long)m * N + off[k * DE_M + m];
    const int bit = a * DE_T + t;
    // pass 1: totals
    int tpl = 0, fpl = 0;
    for (int j = tid; j < nd; j += DE_BT) {
        const int i = list[j];
        const int mt = (int)((rec_match[i] >> bit) & 1), ig = (int)((rec_ign[i] >> bit) & 1);
        tpl += mt & !ig; fpl += !mt & !ig;
    }
    const int tp_total = de_block_sum(tpl, s_red);
    const int fp_total = de_block_sum(fpl, s_red);
    const double npd = (double)np;
    if (tid == 0) recall[(long)t * KAM + kam] = nd ? (double)tp_total / npd : 0.0;
    __syncthreads();   // the zero fill above precedes every write of pass 2
    // pass 2: chunks from the last, prefix counts from the totals, envelope carried from the later chunks
    int tp_after = 0, fp_after = 0;   // sums over the later chunks
    double carry = 0.0;               // max of pr over the later chunks (pr >= 0)
    const int nchunk = (nd + DE_BT - 1) / DE_BT;
    for (int c = nchunk - 1; c >= 0; --c) {
        const int j = c * DE_BT + tid;
        const bool v = j < nd;
        int tpf = 0, fpf = 0, i = 0;
        if (v) {
            i = list[j];
            const int mt = (int)((rec_match[i] >> bit) & 1), ig = (int)((rec_ign[i] >> bit) & 1);
            tpf = mt & !ig; fpf = !mt & !ig;
        }
        s_tp[tid] = tpf; s_fp[tid] = fpf;
        __syncthreads();
        for (int o = 1; o < DE_BT; o <<= 1) {
            const int a1 = tid >= o ? s_tp[tid - o] : 0, b1 = tid >= o ? s_fp[tid - o] : 0;
            __syncthreads();
            s_tp[tid] += a1; s_fp[tid] += b1;
            __syncthreads();
        }
        const int tp_c = s_tp[DE_BT - 1], fp_c = s_fp[DE_BT - 1];
        const int tp_j = tp_total - tp_after - tp_c + s_tp[tid], fp_j = fp_total - fp_after - fp_c + s_fp[tid];
        const double tpd = (double)tp_j, fpd = (double)fp_j;
        const double pr = v ? tpd / (fpd + tpd + 0x1p-52) : 0.0;   // tp / (fp + tp + np.spacing(1))
        s_env[tid] = pr;
        __syncthreads();
        for (int o = 1; o < DE_BT; o <<= 1) {   // suffix max
            const double x = tid + o < DE_BT ? s_env[tid + o] : 0.0;
            __syncthreads();
            s_env[tid] = fmax(s_env[tid], x);
            __syncthreads();
        }
        const double env = fmax(s_env[tid], carry);
        if (v && (tpf || j == 0)) {
            // searchsorted(rc, recThrs, 'left') lands on j for the thresholds in (rc[j-1], rc[j]]
            const double rc = tpd / npd;
            const double rc_prev = j == 0 ? -1.0 : (double)(tp_j - tpf) / npd;
            const double sc = rec_score[i];
            for (int r = 0; r < DE_R; ++r) {
                const double th = s_thr[r];
                if (th > rc_prev && th <= rc) {
                    precision[((long)t * DE_R + r) * KAM + kam] = env;
                    scores[((long)t * DE_R + r) * KAM + kam] = sc;
                }
            }
        }
        const double cmax = fmax(s_env[0], carry);
        __syncthreads();
        carry = cmax;
        tp_after += tp_c; fp_after += fp_c;
    }
}

// ------------------------------------------------------------------------------------------------------------------ C ABI
// mode: 0 bbox, 1 segm, 2 boundary (segm + the boundary planes, their pixel counts and the GT rectangles)
static size_t det_img_workspace_bytes(int num_det, int num_rows, int num_gt, int height, int width, int segm)
{
    if (num_det < 0 || num_rows < 1 || num_gt < 0 || height < 1 || width < 1) return 0;
    const size_t plane = (size_t)width * (((size_t)height + 63) / 64) * 8;
    const size_t nplanes = std::min((size_t)num_det, (size_t)DE_MAXDET * num_rows);   // evaluated dets only
    size_t b = de_align(sizeof(int) * ((size_t)num_rows * (DE_MAXDET + 1) + 1)) + de_align(sizeof(int) * ((size_t)num_det + 1))
             + de_align(sizeof(double) * DE_MAXDET * (size_t)num_gt + 8) + de_align((size_t)DE_A * DE_T * num_gt + 1);
    if (segm) b += de_align(sizeof(int) * 6 * ((size_t)num_det + 1)) + plane * nplanes + de_align(sizeof(int) * ((size_t)num_gt + 1)) + plane * num_gt;
    if (segm == 2) b += de_align(sizeof(int) * ((size_t)num_det + 1)) + plane * nplanes + de_align(sizeof(int) * 5 * ((size_t)num_gt + 1)) + plane * num_gt;
    return b;
}

extern "C" size_t upsnet_det_eval_image_workspace_bytes(int num_det, int num_rows, int num_gt, int height, int width, int segm)
{
    return det_img_workspace_bytes(num_det, num_rows, num_gt, height, width, segm ? 1 : 0);
}

extern "C" size_t upsnet_det_eval_boundary_image_workspace_bytes(int num_det, int num_rows, int num_gt, int height, int width)
{
    return det_img_workspace_bytes(num_det, num_rows, num_gt, height, width, 2);
}

struct DetImgLayout {
    int *slot, *nd, *nplanes, *rank, *plane_of, *det_rect, *det_area, *gt_area, *det_barea, *gt_barea, *gt_rect;
    double *ious;
    unsigned char *gtm;
    de_u64 *det_planes, *gt_planes, *det_bnd, *gt_bnd;
};

static DetImgLayout det_img_layout(void *ws, int n, int K, int G, int H, int W, int segm)
{
    DetImgLayout L = {};
    char *p = (char *)ws;
    size_t o = 0;
    const size_t plane = (size_t)W * ((H + 63) / 64) * 8;
    L.slot = (int *)(p + o); L.nd = L.slot + (size_t)K * DE_MAXDET; L.nplanes = L.nd + K;
    o += de_align(sizeof(int) * ((size_t)K * (DE_MAXDET + 1) + 1));
    L.rank = (int *)(p + o); o += de_align(sizeof(int) * (n + 1));
    L.ious = (double *)(p + o); o += de_align(sizeof(double) * DE_MAXDET * (size_t)G + 8);
    L.gtm = (unsigned char *)(p + o); o += de_align((size_t)DE_A * DE_T * G + 1);
    if (segm) {
        L.det_rect = (int *)(p + o); L.det_area = L.det_rect + 4 * (size_t)(n + 1); L.plane_of = L.det_area + (n + 1);
        o += de_align(sizeof(int) * 6 * (size_t)(n + 1));
        L.det_planes = (de_u64 *)(p + o); o += plane * std::min((size_t)n, (size_t)DE_MAXDET * K);
        L.gt_area = (int *)(p + o); o += de_align(sizeof(int) * (G + 1));
        L.gt_planes = (de_u64 *)(p + o); o += plane * G;
    }
    if (segm == 2) {
        L.det_barea = (int *)(p + o); o += de_align(sizeof(int) * (size_t)(n + 1));
        L.det_bnd = (de_u64 *)(p + o); o += plane * std::min((size_t)n, (size_t)DE_MAXDET * K);
        L.gt_barea = (int *)(p + o); L.gt_rect = L.gt_barea + (G + 1); o += de_align(sizeof(int) * 5 * (size_t)(G + 1));
        L.gt_bnd = (de_u64 *)(p + o); o += plane * G;
    }
    return L;
}

// segm: 0 bbox, 1 segm, 2 boundary with dilation d
static int det_eval_image(void *stream, int segm, int dilation, int height, int width, int num_rows, int num_det, const double *det_xyxy,
                          const double *det_score, const int64_t *det_cls, const int *class_to_row, int num_classes,
                          const float *det_box_f32, const float *mask_prob, int num_mask_channels, int mask_size,
                          const int *det_trans, const int64_t *det_trans_off, int num_gt, const int *gt_row_off,
                          const double *gt_box, const double *gt_area, const int *gt_crowd, const int *gt_trans,
                          const int64_t *gt_trans_off, const int *gt_trans_dst, int num_gt_rle, const unsigned char *const *gt_u8,
                          const int *gt_u8_dst, int num_gt_u8, const int *rows_with_gt, int num_rows_with_gt,
                          const double *params, int image_index, void *workspace, double *rec_score, int *rec_img, int *rec_rk,
                          uint64_t *rec_match, uint64_t *rec_ign, int64_t *npig)
{
    hipStream_t st = (hipStream_t)stream;
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "det_eval_image: bad image size %dx%d", height, width);
    UPS_REQUIRE(num_rows >= 1 && num_rows < (1 << 22) && num_det >= 0 && num_gt >= 0 && num_classes >= 1, "det_eval_image: bad counts");
    UPS_REQUIRE(workspace && gt_row_off && params && rec_score && rec_img && rec_rk && rec_match && rec_ign && npig && class_to_row,
                "det_eval_image: null pointer");
    UPS_REQUIRE(num_det == 0 || (det_score && det_cls), "det_eval_image: null detection pointer");
    UPS_REQUIRE(num_gt == 0 || (gt_area && gt_crowd), "det_eval_image: null GT pointer");
    if (!segm) UPS_REQUIRE((num_det == 0 || det_xyxy) && (num_gt == 0 || gt_box), "det_eval_image: bbox needs boxes");
    if (segm) {
        UPS_REQUIRE(num_det == 0 || (det_box_f32 && mask_prob) || (det_trans && det_trans_off), "det_eval_image: segm needs det masks");
        UPS_REQUIRE(!mask_prob || (num_mask_channels >= 1 && mask_size >= 2 && mask_size + 2 <= IMP_MAXMS), "det_eval_image: bad mask shape");
        UPS_REQUIRE(num_gt_rle + num_gt_u8 == num_gt && (num_gt_rle == 0 || (gt_trans && gt_trans_off && gt_trans_dst))
                    && (num_gt_u8 == 0 || (gt_u8 && gt_u8_dst)), "det_eval_image: every GT needs one mask");
    }
    const int K = num_rows, n = num_det, G = num_gt, H = height, W = width;
    BndTile tile = {};
    if (segm == 2) UPS_REQUIRE(dilation >= 1 && bnd_tile(H, W, dilation, &tile), "det_eval_boundary_image: dilation %d out of range", dilation);
    DetImgLayout L = det_img_layout(workspace, n, K, G, H, W, segm);
    hipLaunchKernelGGL(det_zero_kernel, dim3((K + 1 + DE_BT - 1) / DE_BT), dim3(DE_BT), 0, st, L.nd, K + 1);   // nd and the plane counter
    UPS_CHECK_LAUNCH("det_zero_kernel");
    if (n > 0) {
        hipLaunchKernelGGL(det_rank_kernel, dim3((n + DE_BT - 1) / DE_BT), dim3(DE_BT), 0, st, n, det_score, det_cls, class_to_row,
                           num_classes, image_index, L.rank, L.slot, L.nd, L.plane_of, L.nplanes, rec_score, rec_img, rec_rk);
        UPS_CHECK_LAUNCH("det_rank_kernel");
    }
    const int nw = (H + 63) >> 6;
    const long words = (long)W * nw;
    if (segm) {
        if (G > 0) UPS_CHECK_HIP(hipMemsetAsync(L.gt_area, 0, sizeof(int) * G, st));
        if (n > 0 && mask_prob) {
            hipLaunchKernelGGL(det_paste_kernel, dim3(n), dim3(DE_BT), 0, st, det_box_f32, mask_prob, det_cls, L.plane_of, num_mask_channels,
                               mask_size, H, W, L.det_planes, L.det_rect, L.det_area);
            UPS_CHECK_LAUNCH("det_paste_kernel");
        } else if (n > 0) {
            // run-length dets: the evaluated ones only, each into its plane
            UPS_CHECK_HIP(hipMemsetAsync(L.det_area, 0, sizeof(int) * n, st));
            hipLaunchKernelGGL(det_pack_rle_kernel, dim3((unsigned)((words + DE_BT - 1) / DE_BT), n), dim3(DE_BT), 0, st, det_trans,
                               det_trans_off, (const int *)nullptr, L.plane_of, H, W, L.det_planes, L.det_rect,
                               L.det_area);
            UPS_CHECK_LAUNCH("det_pack_rle_kernel");
        }
        if (segm == 2 && G > 0) {   // the GT rectangles: the run-length GTs write their column range below, a uint8 GT keeps the whole plane
            hipLaunchKernelGGL(bnd_full_rect_kernel, dim3((G + DE_BT - 1) / DE_BT), dim3(DE_BT), 0, st, L.gt_rect, G, W, nw);
            UPS_CHECK_LAUNCH("bnd_full_rect_kernel");
        }
        if (num_gt_rle > 0) {
            hipLaunchKernelGGL(det_pack_rle_kernel, dim3((unsigned)((words + DE_BT - 1) / DE_BT), num_gt_rle), dim3(DE_BT), 0, st, gt_trans,
                               gt_trans_off, gt_trans_dst, (const int *)nullptr, H, W, L.gt_planes, L.gt_rect,
                               L.gt_area);
            UPS_CHECK_LAUNCH("det_pack_rle_kernel");
        }
        for (int j = 0; j < num_gt_u8; ++j) {
            hipLaunchKernelGGL(det_pack_u8_kernel, dim3((unsigned)((words + DE_BT - 1) / DE_BT)), dim3(DE_BT), 0, st, gt_u8[j], gt_u8_dst[j],
                               H, W, L.gt_planes, L.gt_area);
            UPS_CHECK_LAUNCH("det_pack_u8_kernel");
        }
        if (segm == 2 && num_rows_with_gt > 0 && n > 0) {   // (no GT or no det: no IoU is taken, no boundary is needed)
            if (bnd_launch(st, tile, L.det_planes, L.det_rect, L.plane_of, n, H, W, L.det_bnd, L.det_barea)) return 1;
            if (bnd_launch(st, tile, L.gt_planes, L.gt_rect, (const int *)nullptr, G, H, W, L.gt_bnd, L.gt_barea)) return 1;
        }
    }
    if (num_rows_with_gt > 0 && n > 0) {
        UPS_REQUIRE(rows_with_gt, "det_eval_image: null row list");
        hipLaunchKernelGGL(det_iou_kernel, dim3(DE_MAXDET, num_rows_with_gt), dim3(DE_BT), 0, st, segm, rows_with_gt, L.slot, L.nd, det_xyxy,
                           L.det_rect, L.det_area, L.plane_of, L.det_planes, gt_row_off, gt_box, gt_crowd, L.gt_planes, L.gt_area, H, W, L.ious,
                           L.det_bnd, L.det_barea, L.gt_bnd, L.gt_barea, L.gt_rect);
        UPS_CHECK_LAUNCH("det_iou_kernel");
    }
    hipLaunchKernelGGL(det_match_kernel, dim3(K), dim3(UPS_WAVE), 0, st, segm, L.slot, L.nd, det_xyxy, L.det_area, gt_row_off, gt_area,
                       gt_crowd, L.ious, params, L.gtm, (de_u64 *)rec_match, (de_u64 *)rec_ign, npig);
    UPS_CHECK_LAUNCH("det_match_kernel");
    return 0;
}

extern "C" int upsnet_det_eval_image(void *stream, int segm, int height, int width, int num_rows, int num_det, const double *det_xyxy,
                                     const double *det_score, const int64_t *det_cls, const int *class_to_row, int num_classes,
                                     const float *det_box_f32, const float *mask_prob, int num_mask_channels, int mask_size,
                                     const int *det_trans, const int64_t *det_trans_off, int num_gt, const int *gt_row_off,
                                     const double *gt_box, const double *gt_area, const int *gt_crowd, const int *gt_trans,
                                     const int64_t *gt_trans_off, const int *gt_trans_dst, int num_gt_rle, const unsigned char *const *gt_u8,
                                     const int *gt_u8_dst, int num_gt_u8, const int *rows_with_gt, int num_rows_with_gt,
                                     const double *params, int image_index, void *workspace, double *rec_score, int *rec_img, int *rec_rk,
                                     uint64_t *rec_match, uint64_t *rec_ign, int64_t *npig)
{
    return det_eval_image(stream, segm ? 1 : 0, 0, height, width, num_rows, num_det, det_xyxy, det_score, det_cls, class_to_row, num_classes,
                          det_box_f32, mask_prob, num_mask_channels, mask_size, det_trans, det_trans_off, num_gt, gt_row_off, gt_box, gt_area,
                          gt_crowd, gt_trans, gt_trans_off, gt_trans_dst, num_gt_rle, gt_u8, gt_u8_dst, num_gt_u8, rows_with_gt,
                          num_rows_with_gt, params, image_index, workspace, rec_score, rec_img, rec_rk, rec_match, rec_ign, npig);
}

extern "C" int upsnet_det_eval_boundary_image(void *stream, int dilation, int height, int width, int num_rows, int num_det,
                                              const double *det_score, const int64_t *det_cls, const int *class_to_row, int num_classes,
                                              const float *det_box_f32, const float *mask_prob, int num_mask_channels, int mask_size,
                                              const int *det_trans, const int64_t *det_trans_off, int num_gt, const int *gt_row_off,
                                              const double *gt_area, const int *gt_crowd, const int *gt_trans,
                                              const int64_t *gt_trans_off, const int *gt_trans_dst, int num_gt_rle,
                                              const unsigned char *const *gt_u8, const int *gt_u8_dst, int num_gt_u8, const int *rows_with_gt,
                                              int num_rows_with_gt, const double *params, int image_index, void *workspace, double *rec_score,
                                              int *rec_img, int *rec_rk, uint64_t *rec_match, uint64_t *rec_ign, int64_t *npig)
{
    return det_eval_image(stream, 2, dilation, height, width, num_rows, num_det, nullptr, det_score, det_cls, class_to_row, num_classes,
                          det_box_f32, mask_prob, num_mask_channels, mask_size, det_trans, det_trans_off, num_gt, gt_row_off, nullptr, gt_area,
                          gt_crowd, gt_trans, gt_trans_off, gt_trans_dst, num_gt_rle, gt_u8, gt_u8_dst, num_gt_u8, rows_with_gt,
                          num_rows_with_gt, params, image_index, workspace, rec_score, rec_img, rec_rk, rec_match, rec_ign, npig);
}

// ------------------------------------------------------------------------------------------------------------------ boundary masks
extern "C" int upsnet_boundary_dilation_fits(int height, int width, int dilation)
{
    BndTile t;
    return height >= 1 && width >= 1 && dilation >= 1 && bnd_tile(height, width, dilation, &t) ? 1 : 0;
}

extern "C" size_t upsnet_boundary_masks_workspace_bytes(int num_masks, int height, int width)
{
    if (num_masks < 0 || height < 1 || width < 1) return 0;
    const size_t plane = (size_t)width * (((size_t)height + 63) / 64) * 8;
    return 2 * plane * num_masks + de_align(sizeof(int) * 5 * ((size_t)num_masks + 1));
}

extern "C" int upsnet_boundary_masks(void *stream, int dilation, int height, int width, int num_masks, const unsigned char *masks_u8,
                                     const int *trans, const int64_t *trans_off, void *workspace, unsigned char *boundary_u8,
                                     int *boundary_area)
{
    hipStream_t st = (hipStream_t)stream;
    const int n = num_masks, H = height, W = width, nw = (H + 63) >> 6;
    UPS_REQUIRE(H > 0 && W > 0 && (long)H * W < (1L << 31) && n >= 0, "boundary_masks: bad sizes %d x %dx%d", n, H, W);
    BndTile tile = {};
    UPS_REQUIRE(dilation >= 1 && bnd_tile(H, W, dilation, &tile), "boundary_masks: dilation %d out of range", dilation);
    if (n == 0) return 0;
    UPS_REQUIRE(workspace && boundary_u8 && boundary_area && (masks_u8 || (trans && trans_off)), "boundary_masks: null pointer");
    const long words = (long)W * nw;
    de_u64 *planes = (de_u64 *)workspace, *bnd = planes + (size_t)n * words;
    int *area = (int *)(bnd + (size_t)n * words), *rect = area + (n + 1);
    const unsigned nb = (unsigned)((words + DE_BT - 1) / DE_BT);
    UPS_CHECK_HIP(hipMemsetAsync(area, 0, sizeof(int) * n, st));
    hipLaunchKernelGGL(bnd_full_rect_kernel, dim3((n + DE_BT - 1) / DE_BT), dim3(DE_BT), 0, st, rect, n, W, nw);
    UPS_CHECK_LAUNCH("bnd_full_rect_kernel");
    if (masks_u8) {
        for (int p = 0; p < n; ++p) {
            hipLaunchKernelGGL(det_pack_u8_kernel, dim3(nb), dim3(DE_BT), 0, st, masks_u8 + (size_t)p * H * W, p, H, W, planes, area);
            UPS_CHECK_LAUNCH("det_pack_u8_kernel");
        }
    } else {
        UPS_REQUIRE(n <= 65535, "boundary_masks: %d masks in one call (at most 65535)", n);
        hipLaunchKernelGGL(det_pack_rle_kernel, dim3(nb, n), dim3(DE_BT), 0, st, trans, trans_off, (const int *)nullptr, (const int *)nullptr,
                           H, W, planes, rect, area);
        UPS_CHECK_LAUNCH("det_pack_rle_kernel");
    }
    if (bnd_launch(st, tile, planes, rect, (const int *)nullptr, n, H, W, bnd, boundary_area)) return 1;
    hipLaunchKernelGGL(bnd_unpack_u8_kernel, dim3(nb, n), dim3(DE_BT), 0, st, bnd, rect, H, W, boundary_u8);
    UPS_CHECK_LAUNCH("bnd_unpack_u8_kernel");
    return 0;
}

extern "C" size_t upsnet_det_eval_accumulate_workspace_bytes(long num_records, int num_rows)
{
    if (num_records < 0 || num_rows < 1) return 0;
    size_t b = 0;
    det_acc_layout(nullptr, num_records, num_rows, &b);
    return b;
}

extern "C" int upsnet_det_eval_accumulate(void *stream, long num_records, const double *rec_score, const int *rec_img, const int *rec_rk,
                                          const uint64_t *rec_match, const uint64_t *rec_ign, const int *img_ord, int num_rows,
                                          const int64_t *npig, const double *rec_thrs, void *workspace, double *precision, double *recall,
                                          double *scores)
{
    hipStream_t st = (hipStream_t)stream;
    UPS_REQUIRE(num_records >= 0 && num_records < (1L << 31) && num_rows >= 1 && num_rows < (1 << 22), "det_eval_accumulate: bad counts");
    UPS_REQUIRE(workspace && npig && rec_thrs && precision && recall && scores, "det_eval_accumulate: null pointer");
    UPS_REQUIRE(num_records == 0 || (rec_score && rec_img && rec_rk && rec_match && rec_ign && img_ord), "det_eval_accumulate: null record");
    const long N = num_records;
    const int K = num_rows;
    DetAccLayout L = det_acc_layout(workspace, N, K, nullptr);
    hipLaunchKernelGGL(det_zero_kernel, dim3((K * DE_M + DE_BT - 1) / DE_BT), dim3(DE_BT), 0, st, L.cnt, K * DE_M);
    UPS_CHECK_LAUNCH("det_zero_kernel");
    const unsigned nb = (unsigned)((N + DE_BT - 1) / DE_BT);
    if (N > 0) {
        hipLaunchKernelGGL(det_count_kernel, dim3(nb), dim3(DE_BT), 0, st, N, rec_rk, L.cnt);
        UPS_CHECK_LAUNCH("det_count_kernel");
    }
    hipLaunchKernelGGL(det_scan_kernel, dim3(1), dim3(DE_BT), 0, st, K, L.cnt, L.off, L.fill, L.total);
    UPS_CHECK_LAUNCH("det_scan_kernel");
    if (N > 0) {
        hipLaunchKernelGGL(det_scatter_kernel, dim3(nb), dim3(DE_BT), 0, st, N, rec_score, rec_img, rec_rk, img_ord, L.off, L.fill, L.bscore,
                           L.bucket, L.bkey);
        UPS_CHECK_LAUNCH("det_scatter_kernel");
        hipLaunchKernelGGL(det_order_kernel, dim3(nb), dim3(DE_BT), 0, st, K, rec_rk, L.cnt, L.off, L.total, L.bscore, L.bucket, L.bkey,
                           L.sorted, N);
        UPS_CHECK_LAUNCH("det_order_kernel");
    }
    hipLaunchKernelGGL(det_curve_kernel, dim3(K * DE_A * DE_M * DE_T), dim3(DE_BT), 0, st, K, npig, L.cnt, L.off, L.sorted, N, rec_score,
                       (const de_u64 *)rec_match, (const de_u64 *)rec_ign, rec_thrs, precision, recall, scores);
    UPS_CHECK_LAUNCH("det_curve_kernel");
    return 0;
}
