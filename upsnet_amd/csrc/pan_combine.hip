// pan_combine.hip -- BaseDataset.get_combined_pan_result (upsnet/dataset/base_dataset.py:373-449): the heuristic panoptic merge of
// the instance masks (pasted greedily in score order) with the semantic map.
//
// The host (ops.combined_pan_result) decodes the compressed RLE strings (vectorised numpy, no per-character loop), drops the
// candidates below the score threshold and those of zero area, orders them, and cuts every run of ones into segments that do not
// cross a 4096-pixel (64-word) boundary of the column-major pixel index p = x * H + y. Per call, all images of a chunk at once:
//   cpan_hist_kernel    (blocks, image): 256-bin histogram of the uint8 semantic map, LDS-privatised (stuff areas)
//   cpan_greedy_kernel  one workgroup per image, candidates in merge order: remain = popcount(mask & ~occupied) over the segments
//                       (one thread per segment, at most 64 words each), a block reduction, the acceptance rule (thread 0, per-class
//                       instance counters in LDS), then, if accepted, the segments ORed into the occupancy bit plane and the
//                       (category, instance) byte pair written into the owner plane for the newly claimed pixels only
//   cpan_merge_kernel   64 x 64 tiles: owner / occupancy read column-major into LDS, transposed, the stuff-area filter and the
//                       thing / instance rules applied, uint8 [H,W,3] written row-major
// Integers everywhere except the acceptance quotient (float32, compared in double), so the output is exact by construction.
#include "common.h"
#include "upsnet_hip.h"

#define CP_BT 256          // threads per workgroup
#define CP_TILE 64         // merge tile edge
#define CP_HIST_PIX 4096   // pixels per histogram workgroup

typedef unsigned long long cp_u64;

// image table row (int64 [n][CP_IMG_COLS]): height, width, seg (device address), out (device address), first candidate, end of
// candidates, occupancy word offset, pixel offset (owner plane)
#define CP_IMG_COLS 8

__device__ static inline cp_u64 cp_load(const cp_u64 *p)
{
    // occupancy words are also updated with atomics (performed at L2): read them coherently
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(CP_BT)
cpan_hist_kernel(const int64_t *__restrict__ images, int *__restrict__ hist)
{
    __shared__ int s_hist[256];
    const int64_t *im = images + (long)blockIdx.y * CP_IMG_COLS;
    const long npix = im[0] * im[1];
    const long start = (long)blockIdx.x * CP_HIST_PIX;
    if (start >= npix) return;
    const unsigned char *seg = (const unsigned char *)im[2];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const long end = min(start + (long)CP_HIST_PIX, npix);
    for (long i = start + threadIdx.x; i < end; i += CP_BT) atomicAdd(&s_hist[seg[i]], 1);
    __syncthreads();
    const int v = s_hist[threadIdx.x];
    if (v) atomicAdd(&hist[blockIdx.y * 256 + threadIdx.x], v);
}

// bits of word w covered by pixels [a, b) (a < b, the range meets w)
__device__ static inline cp_u64 cp_bits(const long w, const int a, const int b)
{
    const long lo = w << 6;
    const int s = a > lo ? (int)(a - lo) : 0;
    const int e = b < lo + 64 ? (int)(b - lo) : 64;
    return (e - s == 64 ? ~0ull : ((1ull << (e - s)) - 1ull)) << s;
}

// cand int32 [n][4]: class (1-based), area, first segment, end of segments; segs int32 [m][2]: pixel range [a, b) of a run of ones
__global__ void __launch_bounds__(CP_BT)
cpan_greedy_kernel(const int64_t *__restrict__ images, const int *__restrict__ cand, const int *__restrict__ segs,
                   const int id_last_stuff, const double fraction_threshold, cp_u64 *__restrict__ occ_all,
                   unsigned short *__restrict__ owner_all)
{
    __shared__ int s_red[CP_BT / UPS_WAVE];
    __shared__ int s_ins[256];
    __shared__ int s_code;
    const int tid = threadIdx.x;
    const int64_t *im = images + (long)blockIdx.x * CP_IMG_COLS;
    const int c0 = (int)im[4], c1 = (int)im[5];
    cp_u64 *occ = occ_all + im[6];
    unsigned short *owner = owner_all + im[7];
    for (int c = tid; c < 256; c += CP_BT) s_ins[c] = 0;
    __syncthreads();
    for (int k = c0; k < c1; ++k) {
        const int cls = cand[k * 4 + 0], area = cand[k * 4 + 1], sb = cand[k * 4 + 2], se = cand[k * 4 + 3];
        int cnt = 0;
        for (int s = sb + tid; s < se; s += CP_BT) {
            const int a = segs[2 * s], b = segs[2 * s + 1];
            for (long w = a >> 6; w <= (long)((b - 1) >> 6); ++w) cnt += __popcll(cp_bits(w, a, b) & ~cp_load(occ + w));
        }
        for (int o = UPS_WAVE / 2; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, UPS_WAVE);
        if ((tid & (UPS_WAVE - 1)) == 0) s_red[tid / UPS_WAVE] = cnt;
        __syncthreads();
        if (tid == 0) {
            int remain = 0;
            for (int i = 0; i < CP_BT / UPS_WAVE; ++i) remain += s_red[i];
            // fl32(remain / area) < fraction_threshold in double; the double quotient rounded to float equals the float quotient
            // (53 >= 2 * 24 + 2: double rounding is innocuous for division)
            const float q = (float)((double)remain / (double)area);
            int code = -1;
            if (!((double)q < fraction_threshold)) {
                const int ins = ++s_ins[cls];
                code = (id_last_stuff + cls) | (ins << 8);
            }
            s_code = code;
        }
        __syncthreads();
        const int code = s_code;
        if (code >= 0) {
            for (int s = sb + tid; s < se; s += CP_BT) {
                const int a = segs[2 * s], b = segs[2 * s + 1];
                for (long w = a >> 6; w <= (long)((b - 1) >> 6); ++w) {
                    const cp_u64 bits = cp_bits(w, a, b);
                    cp_u64 nb = bits & ~cp_load(occ + w);   // other segments of this candidate own other bits of w
                    if (bits == ~0ull) __hip_atomic_store(occ + w, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    else atomicOr(occ + w, bits);
                    while (nb) {
                        const int i = __ffsll((long long)nb) - 1;
                        owner[(w << 6) + i] = (unsigned short)code;
                        nb &= nb - 1;
                    }
                }
            }
        }
        __syncthreads();   // occupancy complete (and s_red / s_code free) before the next candidate
    }
}

// grid (tiles_x * tiles_y of the largest image, image); tile = CP_TILE columns x CP_TILE rows
__global__ void __launch_bounds__(CP_BT)
cpan_merge_kernel(const int64_t *__restrict__ images, const int tiles_x, const int *__restrict__ hist_all,
                  const cp_u64 *__restrict__ occ_all, const unsigned short *__restrict__ owner_all, const int id_last_stuff,
                  const int stuff_area_limit)
{
    __shared__ unsigned short s_own[CP_TILE][CP_TILE + 1];   // [x][y]
    __shared__ unsigned char s_cat[256];
    const int64_t *im = images + (long)blockIdx.y * CP_IMG_COLS;
    const int H = (int)im[0], W = (int)im[1];
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int x0 = tx * CP_TILE, y0 = ty * CP_TILE;
    if (x0 >= W || y0 >= H) return;
    const unsigned char *seg = (const unsigned char *)im[2];
    unsigned char *out = (unsigned char *)im[3];
    const cp_u64 *occ = occ_all + im[6];
    const unsigned short *owner = owner_all + im[7];
    const int *hist = hist_all + blockIdx.y * 256;
    const int tid = threadIdx.x;
    {
        // semantic value -> category before the instances: stuff under the area limit -> 255, things -> 255 (claimed pixels
        // are overwritten below), other stuff kept
        const int v = tid;
        s_cat[v] = (unsigned char)(v <= id_last_stuff ? (hist[v] < stuff_area_limit ? 255 : v) : 255);
    }
    // read: y fastest (column-major planes)
    for (int i = tid; i < CP_TILE * CP_TILE; i += CP_BT) {
        const int ly = i & (CP_TILE - 1), lx = i >> 6;
        const int x = x0 + lx, y = y0 + ly;
        unsigned short v = 0;
        if (x < W && y < H) {
            const long p = (long)x * H + y;
            if ((occ[p >> 6] >> (p & 63)) & 1ull) v = owner[p];
        }
        s_own[lx][ly] = v;
    }
    __syncthreads();
    // write: x fastest (row-major output)
    for (int i = tid; i < CP_TILE * CP_TILE; i += CP_BT) {
        const int lx = i & (CP_TILE - 1), ly = i >> 6;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const long q = (long)y * W + x;
        const unsigned short v = s_own[lx][ly];
        unsigned char c = s_cat[seg[q]], ins = 0;
        if (v) { c = (unsigned char)(v & 255); ins = (unsigned char)(v >> 8); }
        out[3 * q] = c;
        out[3 * q + 1] = ins;
        out[3 * q + 2] = 0;
    }
}

static inline size_t cp_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t upsnet_combined_pan_workspace_bytes(int num_images, long total_pixels)
{
    if (num_images <= 0 || total_pixels < 0) return 0;
    const size_t hist = cp_align((size_t)num_images * 256 * sizeof(int));
    const size_t occ = cp_align(((size_t)total_pixels / 64 + (size_t)num_images) * sizeof(cp_u64));
    return hist + occ + cp_align((size_t)total_pixels * sizeof(unsigned short));
}

extern "C" int upsnet_combined_pan_result(void *stream, int num_images, const int64_t *images, int max_height, int max_width,
                                          long total_pixels, const int *cand, const int *segments, int id_last_stuff,
                                          int num_classes, int stuff_area_limit, double fraction_threshold, void *workspace)
{
    UPS_REQUIRE(images && workspace, "combined_pan_result: null pointer");
    UPS_REQUIRE(num_images > 0 && max_height > 0 && max_width > 0 && total_pixels > 0 && total_pixels < (1L << 40),
                "combined_pan_result: bad image counts / sizes");
    UPS_REQUIRE((long)max_height * max_width <= (1L << 24), "combined_pan_result: an image of more than 2^24 pixels");
    UPS_REQUIRE(num_classes >= 2 && num_classes <= 256 && id_last_stuff >= 0 && id_last_stuff + num_classes - 1 < 255,
                "combined_pan_result: bad class counts (id_last_stuff %d, num_classes %d)", id_last_stuff, num_classes);
    UPS_REQUIRE(num_images <= 65535, "combined_pan_result: %d images in one call (at most 65535)", num_images);
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const size_t hist_b = cp_align((size_t)num_images * 256 * sizeof(int));
    const size_t occ_b = cp_align(((size_t)total_pixels / 64 + (size_t)num_images) * sizeof(cp_u64));
    int *hist = (int *)ws;
    cp_u64 *occ = (cp_u64 *)(ws + hist_b);
    unsigned short *owner = (unsigned short *)(ws + hist_b + occ_b);
    if (ups_zero_async(ws, hist_b + occ_b, st)) return 1;   // the owner plane is read only where the occupancy bit is set
    const int hist_blocks = ups_divup((long)max_height * max_width, CP_HIST_PIX);
    hipLaunchKernelGGL(cpan_hist_kernel, dim3((unsigned)hist_blocks, (unsigned)num_images), dim3(CP_BT), 0, st, images, hist);
    UPS_CHECK_LAUNCH("cpan_hist_kernel");
    if (cand && segments) {
        hipLaunchKernelGGL(cpan_greedy_kernel, dim3((unsigned)num_images), dim3(CP_BT), 0, st, images, cand, segments, id_last_stuff,
                           fraction_threshold, occ, owner);
        UPS_CHECK_LAUNCH("cpan_greedy_kernel");
    }
    const int tiles_x = ups_divup(max_width, CP_TILE), tiles_y = ups_divup(max_height, CP_TILE);
    hipLaunchKernelGGL(cpan_merge_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)num_images), dim3(CP_BT), 0, st, images, tiles_x,
                       hist, occ, owner, id_last_stuff, stuff_area_limit);
    UPS_CHECK_LAUNCH("cpan_merge_kernel");
    return 0;
}
