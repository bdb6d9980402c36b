// cs_inst_format.hip -- Cityscapes instance predictions in benchmark format, the per-pixel part: the column-major run lists of one
// image's masks (what dataset/cityscapes_eval._transitions yields, what cs_inst_eval.hip walks) expanded into the row-major planes
// the mask PNGs hold. Rules and file layout: dataset/cityscapes_inst_format.py and DESIGN 4.16.
//
//   trans int [off[n]]: per mask the non-decreasing column-major positions p = x * H + y in [0, H * W) at which the mask changes;
//   pixel p is inside when the number of its mask's entries <= p is odd (equal entries cancel: a run of no pixels).
//   8-bit form: out uint8 [n][H][W], 0 / 255.   1-bit form: out uint8 [n][H][ceil(W / 8)], the leftmost pixel of a byte in its most
//   significant bit, the bits past W zero (the row layout of a PNG of bit depth 1).
// One launch per form, no atomics, no workspace, every byte of `out` written exactly once and nothing else.
//   if_expand8_kernel<CPL>  a workgroup owns IF_ROWS rows x 256 * CPL columns of one mask, a lane CPL adjacent columns. The lane finds
//                           its start state by a binary search of the mask's run list for column * H + first row and walks down the
//                           rows, consuming the entries it passes; per row the lanes of a wave store consecutive bytes of the plane.
//                           CPL = 4 (W a multiple of 4, `out` 4-byte aligned): one 4-byte store per lane and row, 256 bytes per wave.
//                           CPL = 1 otherwise: one byte per lane and row.
//   if_expand1_kernel       a workgroup owns IF_ROWS1 rows x 256 columns, a lane one column, walked as above. A wave's 64 columns of
//                           a row are one ballot; its bytes, each bit-reversed, are the eight output bytes. The waves park them in LDS
//                           ([row][wave]: the 32 bytes of a row in output order), and the workgroup stores the tile with 4-byte
//                           stores (ceil(W / 8) a multiple of 4 and `out` aligned) or byte by byte.
#include "common.h"
#include "upsnet_hip.h"

#define IF_BT 256
#define IF_ROWS 64                      // rows of a workgroup, 8-bit form
#define IF_ROWS1 64                     // rows of a workgroup, 1-bit form
#define IF_NONE 0x7FFFFFFF              // "no further entry": above every position (H * W <= 2^30)
#define IF_MAX_Z 65535                  // masks per launch (gridDim.z)

// first index in [lo, hi) whose entry is >= p
__device__ static inline int if_lower_bound(const int *__restrict__ trans, int lo, int hi, const int p)
{
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (trans[mid] < p) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <int CPL>
__global__ void __launch_bounds__(IF_BT)
if_expand8_kernel(const int *__restrict__ trans, const int *__restrict__ off, const int H, const int W, const int col_bands,
                  unsigned char *__restrict__ out)
{
    const int m = blockIdx.z;
    const int cb = blockIdx.x % col_bands, rb = blockIdx.x / col_bands;
    const int c0 = (cb * IF_BT + threadIdx.x) * CPL;         // (CPL = 4 only with W % 4 == 0: c0 < W covers all four columns)
    const int r0 = rb * IF_ROWS;
    if (c0 >= W) return;
    const int r1 = min(r0 + IF_ROWS, H);
    const int lo = off[m], hi = off[m + 1];
    int idx[CPL], nxt[CPL], pos[CPL];
    unsigned on[CPL];
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        pos[k] = (c0 + k) * H + r0;
        idx[k] = if_lower_bound(trans, lo, hi, pos[k]);
        on[k] = (unsigned)(idx[k] - lo) & 1u;
        nxt[k] = idx[k] < hi ? trans[idx[k]] : IF_NONE;
    }
    unsigned char *p = out + ((size_t)m * H + r0) * W + c0;
    for (int r = r0; r < r1; ++r) {
        unsigned word = 0u;
#pragma unroll
        for (int k = 0; k < CPL; ++k) {
            while (nxt[k] == pos[k]) {
                on[k] ^= 1u;
                ++idx[k];
                nxt[k] = idx[k] < hi ? trans[idx[k]] : IF_NONE;
            }
            ++pos[k];
            word |= (on[k] ? 0xFFu : 0u) << (8 * k);
        }
        if (CPL == 4) *(unsigned *)p = word;
        else *p = (unsigned char)word;
        p += W;
    }
}

__global__ void __launch_bounds__(IF_BT)
if_expand1_kernel(const int *__restrict__ trans, const int *__restrict__ off, const int H, const int W, const int WB, const int col_bands,
                  const bool vec, unsigned char *__restrict__ out)
{
    __shared__ unsigned long long s_bits[IF_ROWS1][IF_BT / UPS_WAVE];
    const int m = blockIdx.z, t = threadIdx.x, lane = t & (UPS_WAVE - 1), wave = t / UPS_WAVE;
    const int cb = blockIdx.x % col_bands, rb = blockIdx.x / col_bands;
    const int c = cb * IF_BT + t;
    const int r0 = rb * IF_ROWS1, r1 = min(r0 + IF_ROWS1, H);
    const int lo = off[m], hi = off[m + 1];
    int idx = hi, nxt = IF_NONE, pos = 0;       // a lane past the right edge holds zero bits: the padding of the last byte
    unsigned on = 0u;
    if (c < W) {
        pos = c * H + r0;
        idx = if_lower_bound(trans, lo, hi, pos);
        on = (unsigned)(idx - lo) & 1u;
        nxt = idx < hi ? trans[idx] : IF_NONE;
    }
    for (int r = r0; r < r1; ++r) {             // (the same trips in every lane of the workgroup)
        while (nxt == pos) {
            on ^= 1u;
            ++idx;
            nxt = idx < hi ? trans[idx] : IF_NONE;
        }
        ++pos;
        const unsigned long long b = __ballot(on != 0u);
        // bit l = column l of the wave; byte j must hold columns 8 j .. 8 j + 7 with the first in bit 7: reverse each byte's bits
        if (lane == 0) s_bits[r - r0][wave] = __builtin_bswap64(__brevll(b));
    }
    __syncthreads();
    const int rows = r1 - r0, byte0 = cb * (IF_BT / 8);
    unsigned char *base = out + ((size_t)m * H + r0) * WB + byte0;
    if (vec) {
        for (int i = t; i < rows * (IF_BT / 32); i += IF_BT) {
            const int row = i / (IF_BT / 32), dw = i % (IF_BT / 32);
            if (byte0 + 4 * dw < WB) *(unsigned *)(base + (size_t)row * WB + 4 * dw) = ((const unsigned *)s_bits[row])[dw];
        }
    } else {
        for (int i = t; i < rows * (IF_BT / 8); i += IF_BT) {
            const int row = i / (IF_BT / 8), b = i % (IF_BT / 8);
            if (byte0 + b < WB) base[(size_t)row * WB + b] = ((const unsigned char *)s_bits[row])[b];
        }
    }
}

extern "C" int upsnet_cs_inst_expand(void *stream, const int *trans, const int *trans_off, int num_masks, int height, int width, int bits,
                                     unsigned char *out)
{
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * (long)width <= (1L << 30), "cs_inst_expand: masks of %d x %d (H * W in 1..2^30)",
                height, width);
    UPS_REQUIRE(bits == 8 || bits == 1, "cs_inst_expand: bits = %d (8 or 1)", bits);
    UPS_REQUIRE(num_masks >= 0, "cs_inst_expand: %d masks", num_masks);
    if (num_masks == 0) return 0;
    UPS_REQUIRE(trans && trans_off && out, "cs_inst_expand: null pointer");
    UPS_REQUIRE((((uintptr_t)trans | (uintptr_t)trans_off) & 3) == 0, "cs_inst_expand: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const int WB = (width + 7) / 8;
    const size_t plane = (size_t)height * (bits == 8 ? width : WB);
    for (int m0 = 0; m0 < num_masks; m0 += IF_MAX_Z) {
        const int nm = num_masks - m0 < IF_MAX_Z ? num_masks - m0 : IF_MAX_Z;
        unsigned char *o = out + (size_t)m0 * plane;
        if (bits == 8) {
            const bool vec = width % 4 == 0 && ((uintptr_t)out & 3) == 0;
            const int col_bands = ups_divup(width, IF_BT * (vec ? 4 : 1));
            const dim3 grid((unsigned)col_bands * (unsigned)ups_divup(height, IF_ROWS), 1, (unsigned)nm);
            if (vec) hipLaunchKernelGGL(if_expand8_kernel<4>, grid, dim3(IF_BT), 0, st, trans, trans_off + m0, height, width, col_bands, o);
            else hipLaunchKernelGGL(if_expand8_kernel<1>, grid, dim3(IF_BT), 0, st, trans, trans_off + m0, height, width, col_bands, o);
            UPS_CHECK_LAUNCH("if_expand8_kernel");
        } else {
            const bool vec = WB % 4 == 0 && ((uintptr_t)out & 3) == 0;
            const int col_bands = ups_divup(width, IF_BT);
            const dim3 grid((unsigned)col_bands * (unsigned)ups_divup(height, IF_ROWS1), 1, (unsigned)nm);
            hipLaunchKernelGGL(if_expand1_kernel, grid, dim3(IF_BT), 0, st, trans, trans_off + m0, height, width, WB, col_bands, vec, o);
            UPS_CHECK_LAUNCH("if_expand1_kernel");
        }
    }
    return 0;
}
