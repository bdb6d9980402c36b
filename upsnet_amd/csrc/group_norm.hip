// group_norm.hip -- GroupNorm(32, C) of NHWC fp32 maps for the heads built with with_norm = 'group_norm' (DESIGN.md 4.15):
//     y = relu?( (x - mean_g) * rstd_g * gamma_c + beta_c  [+ residual | + nearest x2 upsampled residual] )
// with statistics per (sample, group) over C / 32 channels x H W pixels.
//
// A lane owns 4 consecutive channels (one 128-bit load), so a pixel is C / 4 lanes and a group C / 128 of them (1 / 2 / 8 for
// C = 128 / 256 / 1024). A workgroup of GN_THREADS lanes walks GN_THREADS / (C / 4) pixels per step.
//
// Sums are carried in fp64 from the first add on: every lane adds x and x * x of its elements (the square of an fp32 is exact in fp64),
// the lanes of a group are combined by a wave butterfly, the pixel rows of the workgroup through the LDS in row order, the chunks of
// a sample in chunk order. var = E[x^2] - mean^2 is formed in fp64 only (for mean 64, std 1 that costs 12 of 53 bits). No atomics:
// every order is fixed by the shape of the sample alone, so a sample's result does not depend on the grid, on its neighbours in the
// launch or on how many maps share it.
//
//   two-phase form   gn_stats_kernel: one workgroup per (map, sample, chunk of GN_CHUNK pixels) -> 32 x (sum, sum of squares) partials;
//                    gn_apply_kernel: same grid; recombines its sample's partials (fixed order), mean / rstd in LDS, streams its chunk.
//   small form       gn_small_kernel: one workgroup per sample of <= GN_CHUNK pixels (ROI maps): the same walk as one stats chunk,
//                    then the apply pass re-reads the sample (L2); bit-identical to the two-phase form on the same sample.
//   rows form        gn_rows_kernel: H = W = 1 (fc6 rows): half a wave per row, one lane per group, the row stays in registers.
#include <string.h>

#include "common.h"
#include "upsnet_hip.h"

#define GN_GROUPS 32
#define GN_CHUNK 512
#define GN_THREADS 512
#define GN_MAX_SEG 5
#define GN_MAX_C 1024
#define GN_SLICES (GN_THREADS / GN_GROUPS)

struct GnSeg {
    const float *x;
    float *out;
    const float *res;   // NULL, [N, H, W, C] or (res_up) [N, H / 2, W / 2, C]
    int batch, hw, width, nchunk;
    int blk0;           // first workgroup of this map
    long ws0;           // first partial (in double2 units) of this map
};

struct GnParams {
    GnSeg seg[GN_MAX_SEG];
    int nseg, C, relu, res_up;
    float eps;
    const float *gamma, *beta;
    double2 *ws;
};

__device__ static inline void gn_finalize(double s, double q, double count, float eps, float *mean, float *rstd)
{
    double m = s / count;
    double var = q / count - m * m;
    var = var < 0.0 ? 0.0 : var;
    *mean = (float)m;
    *rstd = (float)(1.0 / sqrt(var + (double)eps));
}

// (sum, sum of squares) of `len` pixels x C channels starting at xs, per group: returned to threads 0..31 (thread g: group g).
// red: GN_THREADS double2 of LDS. Every thread of the workgroup must call it.
__device__ static inline double2 gn_chunk_sums(const float *xs, int len, int C, double2 *red)
{
    const int L = C >> 2, R = GN_THREADS / L, lpg = C >> 7;
    const int t = threadIdx.x, cl = t % L, pr = t / L;
    const bool pow2 = (lpg & (lpg - 1)) == 0;
    double s = 0.0, q = 0.0;
    if (pr < R) {
        const float *p = xs + (size_t)pr * C + cl * 4;
        const size_t step = (size_t)R * C;
#pragma unroll 4
        for (int i = pr; i < len; i += R, p += step) {
            const float4 v = *reinterpret_cast<const float4 *>(p);
            const double a = v.x, b = v.y, c = v.z, d = v.w;
            s += (a + b) + (c + d);
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    if (pow2) {   // the lanes of a group are neighbours inside one wave
        for (int m = 1; m < lpg; m <<= 1) {
            s += __shfl_xor(s, m);
            q += __shfl_xor(q, m);
        }
    }
    red[t] = make_double2(s, q);
    __syncthreads();
    double2 tot = make_double2(0.0, 0.0);
    if (t < GN_GROUPS) {
        const int nk = pow2 ? 1 : lpg;
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < nk; ++k) {
                const double2 e = red[r * L + t * lpg + k];
                tot.x += e.x;
                tot.y += e.y;
            }
    }
    __syncthreads();
    return tot;
}

// The apply pass over `len` pixels starting at pixel p0 of one sample. sm / sr: mean / rstd of the 32 groups (LDS).
__device__ static inline void gn_apply_pixels(const float *xs, float *os, const float *rs, int p0, int len, int C, int width, int relu,
                                              int res_up, const float *gamma, const float *beta, const float *sm, const float *sr)
{
    const int L = C >> 2, R = GN_THREADS / L, lpg = C >> 7;
    const int t = threadIdx.x, cl = t % L, pr = t / L;
    if (pr >= R) return;
    const int g = cl / lpg;
    const float mean = sm[g], rstd = sr[g];
    const float4 ga = *reinterpret_cast<const float4 *>(gamma + cl * 4);
    const float4 be = *reinterpret_cast<const float4 *>(beta + cl * 4);
    const float4 a = make_float4(rstd * ga.x, rstd * ga.y, rstd * ga.z, rstd * ga.w);
    const int rw = width >> 1;
#pragma unroll 2
    for (int i = pr; i < len; i += R) {
        const size_t p = (size_t)(p0 + i);
        const float4 v = *reinterpret_cast<const float4 *>(xs + p * C + cl * 4);
        float4 y = make_float4((v.x - mean) * a.x + be.x, (v.y - mean) * a.y + be.y, (v.z - mean) * a.z + be.z, (v.w - mean) * a.w + be.w);
        if (rs) {
            size_t rp = p;
            if (res_up) {
                const int h = (p0 + i) / width, w = (p0 + i) - h * width;
                rp = (size_t)(h >> 1) * rw + (w >> 1);
            }
            const float4 r = *reinterpret_cast<const float4 *>(rs + rp * C + cl * 4);
            y.x += r.x; y.y += r.y; y.z += r.z; y.w += r.w;
        }
        if (relu) {
            y.x = fmaxf(y.x, 0.f); y.y = fmaxf(y.y, 0.f); y.z = fmaxf(y.z, 0.f); y.w = fmaxf(y.w, 0.f);
        }
        *reinterpret_cast<float4 *>(os + p * C + cl * 4) = y;
    }
}

// workgroup -> (map, sample, chunk)
__device__ static inline const GnSeg &gn_locate(const GnParams &P, int *n, int *chunk)
{
    int s = 0;
    for (int i = 1; i < P.nseg; ++i)
        if ((int)blockIdx.x >= P.seg[i].blk0) s = i;
    const GnSeg &S = P.seg[s];
    const int local = (int)blockIdx.x - S.blk0;
    *n = local / S.nchunk;
    *chunk = local - *n * S.nchunk;
    return S;
}

__global__ __launch_bounds__(GN_THREADS) void gn_stats_kernel(const GnParams P)
{
    __shared__ double2 red[GN_THREADS];
    int n, ch;
    const GnSeg &S = gn_locate(P, &n, &ch);
    const int p0 = ch * GN_CHUNK, len = min(GN_CHUNK, S.hw - p0);
    const double2 tot = gn_chunk_sums(S.x + ((size_t)n * S.hw + p0) * P.C, len, P.C, red);
    if (threadIdx.x < GN_GROUPS) P.ws[S.ws0 + ((long)n * S.nchunk + ch) * GN_GROUPS + threadIdx.x] = tot;
}

__global__ __launch_bounds__(GN_THREADS) void gn_apply_kernel(const GnParams P)
{
    __shared__ double2 red[GN_THREADS];
    __shared__ float sm[GN_GROUPS], sr[GN_GROUPS];
    int n, ch;
    const GnSeg &S = gn_locate(P, &n, &ch);
    const int t = threadIdx.x, g = t & (GN_GROUPS - 1), slice = t >> 5;
    // the sample's partials: slice k adds chunks k, k + 16, ... in that order; group g then adds the 16 slices in order
    const double2 *ws = P.ws + S.ws0 + (long)n * S.nchunk * GN_GROUPS;
    double s = 0.0, q = 0.0;
    for (int j = slice; j < S.nchunk; j += GN_SLICES) {
        const double2 e = ws[j * GN_GROUPS + g];
        s += e.x;
        q += e.y;
    }
    red[t] = make_double2(s, q);
    __syncthreads();
    if (t < GN_GROUPS) {
        double ts = 0.0, tq = 0.0;
        for (int k = 0; k < GN_SLICES; ++k) {
            ts += red[k * GN_GROUPS + t].x;
            tq += red[k * GN_GROUPS + t].y;
        }
        gn_finalize(ts, tq, (double)S.hw * (double)(P.C >> 5), P.eps, &sm[t], &sr[t]);
    }
    __syncthreads();
    const int p0 = ch * GN_CHUNK, len = min(GN_CHUNK, S.hw - p0);
    const size_t base = (size_t)n * S.hw * P.C;
    const float *rs = nullptr;
    if (S.res) rs = S.res + (P.res_up ? (size_t)n * (S.hw >> 2) * P.C : base);
    gn_apply_pixels(S.x + base, S.out + base, rs, p0, len, P.C, S.width, P.relu, P.res_up, P.gamma, P.beta, sm, sr);
}

// one workgroup per sample of hw <= GN_CHUNK pixels
__global__ __launch_bounds__(GN_THREADS) void gn_small_kernel(const float *x, float *out, int hw, int C, const float *gamma, const float *beta,
                                                              float eps, int relu)
{
    __shared__ double2 red[GN_THREADS];
    __shared__ float sm[GN_GROUPS], sr[GN_GROUPS];
    const size_t base = (size_t)blockIdx.x * hw * C;
    const double2 tot = gn_chunk_sums(x + base, hw, C, red);
    if (threadIdx.x < GN_GROUPS) {
        // (what gn_apply_kernel makes of a single chunk: slice 0 holds the partial, 0 + partial + 15 zeros)
        gn_finalize(0.0 + tot.x, 0.0 + tot.y, (double)hw * (double)(C >> 5), eps, &sm[threadIdx.x], &sr[threadIdx.x]);
    }
    __syncthreads();
    gn_apply_pixels(x + base, out + base, nullptr, 0, hw, C, 1, relu, 0, gamma, beta, sm, sr);
}

// rows [n, C]: lane (0..31) of each half wave owns one group of C / 32 <= 32 consecutive channels, held in registers
__global__ __launch_bounds__(256) void gn_rows_kernel(const float *x, float *out, int n, int C, const float *gamma, const float *beta, float eps,
                                                      int relu)
{
    const int row = (int)blockIdx.x * 8 + ((int)threadIdx.x >> 5), g = threadIdx.x & 31;
    if (row >= n) return;
    const int nq = C >> 7;   // float4s per group
    const size_t off = (size_t)row * C + (size_t)g * (C >> 5);
    float4 v[8];
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < nq) {
            v[i] = *reinterpret_cast<const float4 *>(x + off + i * 4);
            const double a = v[i].x, b = v[i].y, c = v[i].z, d = v[i].w;
            s += (a + b) + (c + d);
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    float mean, rstd;
    gn_finalize(s, q, (double)(C >> 5), eps, &mean, &rstd);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (i < nq) {
            const float4 ga = *reinterpret_cast<const float4 *>(gamma + g * (C >> 5) + i * 4);
            const float4 be = *reinterpret_cast<const float4 *>(beta + g * (C >> 5) + i * 4);
            float4 y = make_float4((v[i].x - mean) * (rstd * ga.x) + be.x, (v[i].y - mean) * (rstd * ga.y) + be.y,
                                   (v[i].z - mean) * (rstd * ga.z) + be.z, (v[i].w - mean) * (rstd * ga.w) + be.w);
            if (relu) {
                y.x = fmaxf(y.x, 0.f); y.y = fmaxf(y.y, 0.f); y.z = fmaxf(y.z, 0.f); y.w = fmaxf(y.w, 0.f);
            }
            *reinterpret_cast<float4 *>(out + off + i * 4) = y;
        }
    }
}

// ------------------------------------------------------------------------------------------------ host side
static inline bool gn_aligned(const void *p) { return ((uintptr_t)p & 15) == 0; }

static int gn_check_channels(const char *who, int C)
{
    UPS_REQUIRE(C > 0 && C % 128 == 0 && C <= GN_MAX_C,
                "%s: C = %d is not supported (32 groups of whole 128-bit lanes: C %% 128 == 0 and C <= %d)", who, C, GN_MAX_C);
    return 0;
}

extern "C" int upsnet_group_norm_chunk_pixels(void) { return GN_CHUNK; }

extern "C" size_t upsnet_group_norm_workspace_bytes(int nseg, const int batch[], const int height[], const int width[])
{
    if (nseg < 1 || nseg > GN_MAX_SEG || !batch || !height || !width) return 0;
    size_t n = 0;
    for (int i = 0; i < nseg; ++i) {
        if (batch[i] < 0 || height[i] < 0 || width[i] < 0) return 0;
        const long hw = (long)height[i] * width[i];
        n += (size_t)batch[i] * (size_t)((hw + GN_CHUNK - 1) / GN_CHUNK) * GN_GROUPS * sizeof(double2);
    }
    return n;
}

extern "C" int upsnet_group_norm_nhwc_f32(void *stream, int nseg, const float *const x[], float *const out[], const int batch[],
                                          const int height[], const int width[], int C, const float *gamma, const float *beta, float eps,
                                          int relu, const float *const residual[], const int res_height[], const int res_width[],
                                          int residual_up, void *workspace)
{
    const char *who = "group_norm_nhwc_f32";
    UPS_REQUIRE(nseg >= 1 && nseg <= GN_MAX_SEG, "%s: 1..%d maps per launch, got %d", who, GN_MAX_SEG, nseg);
    UPS_REQUIRE(x && out && batch && height && width && gamma && beta, "%s: null pointer", who);
    if (gn_check_channels(who, C)) return 1;
    UPS_REQUIRE(eps >= 0.f, "%s: eps must be >= 0", who);
    UPS_REQUIRE(gn_aligned(gamma) && gn_aligned(beta), "%s: gamma / beta must be 16-byte aligned", who);
    UPS_REQUIRE(!residual || (res_height && res_width), "%s: residual given without its res_height / res_width", who);
    GnParams P;
    memset(&P, 0, sizeof(P));
    long blocks = 0, parts = 0;
    for (int i = 0; i < nseg; ++i) {
        UPS_REQUIRE(batch[i] >= 0 && height[i] >= 0 && width[i] >= 0, "%s: map %d: negative size", who, i);
        const long hw = (long)height[i] * width[i];
        UPS_REQUIRE(hw < (1L << 30), "%s: map %d: %d x %d pixels per sample is too large", who, i, height[i], width[i]);
        const bool empty = batch[i] == 0 || hw == 0;
        UPS_REQUIRE(empty || (x[i] && out[i]), "%s: null pointer (map %d)", who, i);
        UPS_REQUIRE(gn_aligned(x[i]) && gn_aligned(out[i]), "%s: map %d: x / out must be 16-byte aligned", who, i);
        const float *r = residual ? residual[i] : nullptr;
        if (r) {
            UPS_REQUIRE(gn_aligned(r), "%s: map %d: residual must be 16-byte aligned", who, i);
            if (residual_up) {
                UPS_REQUIRE(height[i] % 2 == 0 && width[i] % 2 == 0 && res_height[i] * 2 == height[i] && res_width[i] * 2 == width[i],
                            "%s: map %d: an upsampled residual must be [N, %d / 2, %d / 2, C] with even H, W; got %d x %d", who, i,
                            height[i], width[i], res_height[i], res_width[i]);
                UPS_REQUIRE(r != out[i], "%s: map %d: out may not alias an upsampled residual", who, i);
            } else {
                UPS_REQUIRE(res_height[i] == height[i] && res_width[i] == width[i], "%s: map %d: residual is %d x %d, the map %d x %d", who,
                            i, res_height[i], res_width[i], height[i], width[i]);
            }
        }
        GnSeg &S = P.seg[i];
        S.x = x[i]; S.out = out[i]; S.res = r;
        S.batch = batch[i]; S.hw = (int)hw; S.width = width[i];
        S.nchunk = empty ? 1 : (int)((hw + GN_CHUNK - 1) / GN_CHUNK);
        S.blk0 = (int)blocks;
        S.ws0 = parts;
        if (!empty) {
            blocks += (long)batch[i] * S.nchunk;
            parts += (long)batch[i] * S.nchunk * GN_GROUPS;
        }
        UPS_REQUIRE(blocks < (1L << 30), "%s: too many chunks in one launch", who);
    }
    if (blocks == 0) return 0;
    UPS_REQUIRE(workspace, "%s: null workspace (upsnet_group_norm_workspace_bytes)", who);
    UPS_REQUIRE(gn_aligned(workspace), "%s: workspace must be 16-byte aligned", who);
    P.nseg = nseg; P.C = C; P.relu = relu != 0; P.res_up = residual_up != 0; P.eps = eps;
    P.gamma = gamma; P.beta = beta; P.ws = (double2 *)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gn_stats_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, st, P);
    UPS_CHECK_LAUNCH("gn_stats_kernel");
    hipLaunchKernelGGL(gn_apply_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, st, P);
    UPS_CHECK_LAUNCH("gn_apply_kernel");
    return 0;
}

extern "C" int upsnet_group_norm_small_nhwc_f32(void *stream, const float *x, float *out, int batch, int height, int width, int C,
                                                const float *gamma, const float *beta, float eps, int relu)
{
    const char *who = "group_norm_small_nhwc_f32";
    UPS_REQUIRE(gamma && beta, "%s: null pointer", who);
    if (gn_check_channels(who, C)) return 1;
    UPS_REQUIRE(eps >= 0.f, "%s: eps must be >= 0", who);
    UPS_REQUIRE(batch >= 0 && height >= 0 && width >= 0, "%s: negative size", who);
    const long hw = (long)height * width;
    UPS_REQUIRE(hw <= GN_CHUNK, "%s: %d x %d pixels per sample: this form takes at most %d (upsnet_group_norm_nhwc_f32 takes the rest)", who,
                height, width, GN_CHUNK);
    UPS_REQUIRE(batch < (1 << 30), "%s: batch too large", who);
    if (batch == 0 || hw == 0) return 0;
    UPS_REQUIRE(x && out, "%s: null pointer", who);
    UPS_REQUIRE(gn_aligned(x) && gn_aligned(out) && gn_aligned(gamma) && gn_aligned(beta), "%s: pointers must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    if (hw == 1) {
        hipLaunchKernelGGL(gn_rows_kernel, dim3((unsigned)ups_divup(batch, 8)), dim3(256), 0, st, x, out, batch, C, gamma, beta, eps, relu != 0);
        UPS_CHECK_LAUNCH("gn_rows_kernel");
    } else {
        hipLaunchKernelGGL(gn_small_kernel, dim3((unsigned)batch), dim3(GN_THREADS), 0, st, x, out, (int)hw, C, gamma, beta, eps, relu != 0);
        UPS_CHECK_LAUNCH("gn_small_kernel");
    }
    return 0;
}
