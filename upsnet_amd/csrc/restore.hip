// restore.hip -- the semantic and panoptic label maps of one image brought back to the original image resolution, the step of the
// reference's test loop after the network (upsnet/upsnet_end2end_test.py:258-272): crop to the resized size, astype('uint8'),
// cv2.resize(fx = 1 / im_scale, INTER_NEAREST). The same gather serves the PIL NEAREST resize of evaluate_ssegs
// (cityscapes.py:445-492, coco.py:225-273) when a prediction and its GT label PNG differ in shape.
//
// A nearest-neighbour resize is a pure gather out[y, x] = src[y_ofs[y], x_ofs[x]]: the host builds the two index tables (the cv2 or
// PIL rule, double precision, dataset/restore.py) and one launch writes both output maps. Each thread owns 16 consecutive output
// bytes of the flat row-major output (one 16-byte store when the chunk is whole and aligned); the source row pointer is looked up once
// per output row the chunk touches. The int64 -> uint8 cast keeps the low byte, numpy's astype('uint8') wrap.
#include "common.h"
#include "upsnet_hip.h"

#define RS_CHUNK 16
#define RS_BLOCK 256

// one thread's chunk of the gather from a plane of T (the low byte of an element is kept)
template <class T>
__device__ static inline void rs_gather_chunk(const T *__restrict__ src, const long stride, const int src_h, const int src_w,
                                              const int *__restrict__ y_ofs, const int *__restrict__ x_ofs, const int out_h, const int out_w,
                                              unsigned char *__restrict__ dst)
{
    const long npix = (long)out_h * out_w;
    const long p0 = ((long)blockIdx.x * RS_BLOCK + threadIdx.x) * RS_CHUNK;
    if (p0 >= npix) return;
    int y = (int)(p0 / out_w), x = (int)(p0 - (long)y * out_w);
    const T *row = src + (long)min(max(y_ofs[y], 0), src_h - 1) * stride;
    unsigned w[RS_CHUNK / 4] = {0u, 0u, 0u, 0u};
    const int n = (int)min((long)RS_CHUNK, npix - p0);
#pragma unroll
    for (int j = 0; j < RS_CHUNK; ++j) {
        if (j < n) {
            const int sx = min(max(x_ofs[x], 0), src_w - 1);
            w[j >> 2] |= ((unsigned)row[sx] & 0xffu) << (8 * (j & 3));
            if (++x == out_w && j + 1 < n) {      // next output row: one new row lookup
                x = 0;
                ++y;
                row = src + (long)min(max(y_ofs[y], 0), src_h - 1) * stride;
            }
        }
    }
    unsigned char *o = dst + p0;
    if (n == RS_CHUNK && ((uintptr_t)o & 15) == 0) {
        *(uint4 *)o = make_uint4(w[0], w[1], w[2], w[3]);
    } else if (((uintptr_t)o & 3) == 0) {
        for (int j = 0; j < n / 4; ++j) ((unsigned *)o)[j] = w[j];
        for (int j = n & ~3; j < n; ++j) o[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    } else {
        for (int j = 0; j < n; ++j) o[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    }
}

__global__ void __launch_bounds__(RS_BLOCK)
restore_label_maps_kernel(const int64_t *__restrict__ src0, const int64_t *__restrict__ src1, const long stride, const int src_h,
                          const int src_w, const int *__restrict__ y_ofs, const int *__restrict__ x_ofs, const int out_h, const int out_w,
                          unsigned char *__restrict__ dst0, unsigned char *__restrict__ dst1)
{
    // blockIdx.y selects the map: 0 = semantic, 1 = panoptic (grid.y is 1 when there is no panoptic map)
    rs_gather_chunk(blockIdx.y ? src1 : src0, stride, src_h, src_w, y_ofs, x_ofs, out_h, out_w, blockIdx.y ? dst1 : dst0);
}

// the same gather for a uint8 plane (the panoptic confidence)
__global__ void __launch_bounds__(RS_BLOCK)
restore_plane_u8_kernel(const unsigned char *__restrict__ src, const long stride, const int src_h, const int src_w,
                        const int *__restrict__ y_ofs, const int *__restrict__ x_ofs, const int out_h, const int out_w,
                        unsigned char *__restrict__ dst)
{
    rs_gather_chunk(src, stride, src_h, src_w, y_ofs, x_ofs, out_h, out_w, dst);
}

extern "C" int upsnet_restore_label_maps(void *stream, const int64_t *sseg, const int64_t *pano, long src_stride, int src_height,
                                         int src_width, const int *y_ofs, int out_height, const int *x_ofs, int out_width,
                                         unsigned char *out_sseg, unsigned char *out_pano)
{
    UPS_REQUIRE(sseg && y_ofs && x_ofs && out_sseg, "restore_label_maps: null pointer");
    UPS_REQUIRE(!pano == !out_pano, "restore_label_maps: pano and out_pano must both be given or both be null");
    UPS_REQUIRE(src_height >= 1 && src_width >= 1 && src_stride >= src_width, "restore_label_maps: bad source %d x %d, stride %ld",
                src_height, src_width, src_stride);
    UPS_REQUIRE(out_height >= 0 && out_width >= 0 && (long)out_height * out_width < (1L << 40),
                "restore_label_maps: bad output %d x %d", out_height, out_width);
    const long npix = (long)out_height * out_width;
    if (npix == 0) return 0;
    const long threads = (npix + RS_CHUNK - 1) / RS_CHUNK;
    const long blocks = (threads + RS_BLOCK - 1) / RS_BLOCK;
    UPS_REQUIRE(blocks < (1L << 31), "restore_label_maps: output of %ld pixels too large", npix);
    hipLaunchKernelGGL(restore_label_maps_kernel, dim3((unsigned)blocks, pano ? 2 : 1), dim3(RS_BLOCK), 0, (hipStream_t)stream, sseg,
                       pano, src_stride, src_height, src_width, y_ofs, x_ofs, out_height, out_width, out_sseg, out_pano);
    UPS_CHECK_LAUNCH("restore_label_maps_kernel");
    return 0;
}

extern "C" int upsnet_restore_plane_u8(void *stream, const unsigned char *src, long src_stride, int src_height, int src_width,
                                       const int *y_ofs, int out_height, const int *x_ofs, int out_width, unsigned char *out)
{
    UPS_REQUIRE(src && y_ofs && x_ofs && out, "restore_plane_u8: null pointer");
    UPS_REQUIRE(src_height >= 1 && src_width >= 1 && src_stride >= src_width, "restore_plane_u8: bad source %d x %d, stride %ld", src_height,
                src_width, src_stride);
    UPS_REQUIRE(out_height >= 0 && out_width >= 0 && (long)out_height * out_width < (1L << 40), "restore_plane_u8: bad output %d x %d",
                out_height, out_width);
    const long npix = (long)out_height * out_width;
    if (npix == 0) return 0;
    const long threads = (npix + RS_CHUNK - 1) / RS_CHUNK;
    const long blocks = (threads + RS_BLOCK - 1) / RS_BLOCK;
    UPS_REQUIRE(blocks < (1L << 31), "restore_plane_u8: output of %ld pixels too large", npix);
    hipLaunchKernelGGL(restore_plane_u8_kernel, dim3((unsigned)blocks), dim3(RS_BLOCK), 0, (hipStream_t)stream, src, src_stride, src_height,
                       src_width, y_ofs, x_ofs, out_height, out_width, out);
    UPS_CHECK_LAUNCH("restore_plane_u8_kernel");
    return 0;
}
