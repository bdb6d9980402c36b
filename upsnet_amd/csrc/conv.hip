// conv.hip -- dense AND deformable convolution as one fp32 implicit-GEMM kernel family on the MFMA units of gfx950.
//
// Reference (dense): every nn.Conv2d of the backbone / FPN / RPN / heads (upsnet/models/resnet.py:53-100,
// fpn.py:78-104, rpn.py:52-57, rcnn.py:79-87, fcn.py:88-108) followed by separate frozen-BN, bias, ReLU and
// residual-add passes. Reference (deformable): DeformConvFunction.forward = deformable_im2col into a column
// buffer in HBM + torch.mm + bias (upsnet/operators/functions/deform_conv.py:43-57, deform_conv_kernel.cu:194-242;
// v2: mod_deform_conv_kernel.cu:187-249).
//
// Here: NHWC activations, weights pre-packed once to [kh*kw*Cin, ldw] (tap-major rows, ldw = Cout rounded up to 32,
// zero padded). A workgroup owns BM (64/128) output pixels x BN output channels. K is walked in slabs of one tap x 32 input
// channels. While slab s is contracted from LDS with v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation in a fixed k order), the global loads of slab s+2 (dense) / s+1 (deformable) are already in flight
// into registers (double-buffered LDS, one barrier per slab):
//   dense      : one float4 per (pixel, 4 channels), zero-filled outside the image;
//   deformable : the four bilinear corners as float4 channel runs; offsets -> corner addresses + weights are
//                computed once per tap in registers with the reference's exact fp32 arithmetic; the blend (and the
//                v2 modulation) happens when the registers are written to LDS. No column buffer exists.
// Epilogue fused: + bias (the folded frozen-BN shift), + residual, ReLU, one store.
// Up to 5 feature maps that share the same weights (FPN levels: RPN head, FCN-head subnet) go in ONE launch.
#include "common.h"
#include "upsnet_hip.h"

#include "conv_params.h"
#include "residency.h"

// corner descriptor of one (pixel, tap), kept small (4-5 registers) because the deformable instances are register-bound:
// BYTE offset of the top-left corner (clamped, always loadable; advances by one channel slab per fetch), the bilinear
// fractions, validity bits 0-3 (corner inside the image) and step bits 4-5 (right / lower neighbour is a distinct,
// in-range pixel), v2 modulation. Weights are re-derived at blend time with the reference's exact fp32 expressions
// (deform_conv_kernel.cu:88-118).
struct DcnDesc {
    unsigned o1;
    float lh, lw, m;
    unsigned vb;
};

// nb: element offset of (image n, channel group) of this thread inside the feature map
__device__ static inline DcnDesc dcn_desc(const ConvSeg &sg, const long pp, const int nb, const int tap, const int ntap,
                                          const int h_base, const int w_base, const int cin, const bool mod)
{
    DcnDesc d;
    d.o1 = 4u * (unsigned)nb;
    d.lh = d.lw = 0.f;
    d.m = 1.f;
    d.vb = 0;
    if (pp < 0) return d;
    const float off_h = sg.off[pp * (2 * ntap) + 2 * tap];
    const float off_w = sg.off[pp * (2 * ntap) + 2 * tap + 1];
    const float h_im = (float)h_base + off_h;   // integer part converted to float before the add (:227-228)
    const float w_im = (float)w_base + off_w;
    const int H = sg.H, W = sg.W;
    if (h_im > -1 && w_im > -1 && h_im < (float)H && w_im < (float)W) {
        const int h_low = (int)floorf(h_im), w_low = (int)floorf(w_im);
        const int h_high = h_low + 1, w_high = w_low + 1;
        d.lh = h_im - (float)h_low;
        d.lw = w_im - (float)w_low;
        const bool a = h_low >= 0, b = h_high <= H - 1, c = w_low >= 0, e = w_high <= W - 1;
        const int hl = a ? h_low : 0, wl = c ? w_low : 0;
        d.o1 = 4u * (unsigned)(nb + (hl * W + wl) * cin);
        // right neighbour differs from the left one iff both w_low >= 0 and w_high <= W-1 (otherwise the clamped pair
        // coincides and the invalid one is masked); same for rows
        d.vb = (a && c ? 1u : 0u) | (a && e ? 2u : 0u) | (b && c ? 4u : 0u) | (b && e ? 8u : 0u) |
               (c && e ? 16u : 0u) | (a && b ? 32u : 0u);
    }
    if (mod) d.m = sg.mask[pp * ntap + tap];
    return d;
}

__device__ static inline float dcn_blend1(const DcnDesc &d, float v1, float v2, float v3, float v4, const bool mod)
{
    const float hh = 1.0f - d.lh, hw = 1.0f - d.lw;
    const float w1 = hh * hw, w2 = hh * d.lw, w3 = d.lh * hw, w4 = d.lh * d.lw;
    v1 = (d.vb & 1u) ? v1 : 0.f;
    v2 = (d.vb & 2u) ? v2 : 0.f;
    v3 = (d.vb & 4u) ? v3 : 0.f;
    v4 = (d.vb & 8u) ? v4 : 0.f;
    float val = w1 * v1;
    val = val + w2 * v2;
    val = val + w3 * v3;
    val = val + w4 * v4;
    if (mod) val = val * d.m;
    return val;
}

// WM x WN = 32x32 tiles per wave, waves arranged WAVES_M x WAVES_N (4 waves): BM = 32*WM*WAVES_M (128 or 64) output
// pixels x BN = 32*WN*WAVES_N (128 / 64 / 32) output channels per workgroup. BK = input channels per K slab (32 / 64).
// DEFORM (A-operand loader): 0 dense, 1 deformable v1, 2 deformable v2 (modulated), 3 stem: the input is an NHWC image with
// 4 channels (RGB + zero) and a K slab is one kernel ROW -- 8 consecutive input pixels x 4 channels = 32 contiguous floats --
// so the 7x7/2 stem (Cin = 3) runs on the same MFMA pipeline with K = 7 x 32 instead of a 10x zero-padded K.
// RESUP (epilogue): 0 plain, 1 residual read through a nearest x2 upsampling, 2 deconvolution scatter: the GEMM columns are
// (dy, dx, co) of a 2x2 / stride-2 transposed convolution and each result is stored at output pixel (2h+dy, 2w+dx).
//
// Schedule of one slab (KS = BK/2 MFMA steps per 32x32 tile), pinned with sched_barrier because a wave that runs
// alone on its SIMD (small feature maps) only keeps the MFMA pipe busy if everything else sits in the shadow of an MFMA:
//   step 0        issue the global loads of a later slab (dense: slab s+2 into the register set not in use;
//                 deformable: slab s+1) -- addresses advance incrementally, they are only recomputed at tap changes
//   step k        LDS fragment reads of step k+1, then the MFMAs of step k
//   steps KS-6..  registers of slab s+1 -> the other LDS buffer, one pixel (or the B slab) per step
//   step KS-2     barrier (all fragment reads of this buffer are complete, all stashes visible)
//   step KS-1     fragment reads of step 0 of slab s+1 from the other buffer
template <int WM, int WN, int WAVES_M, int WAVES_N, int DEFORM, int BK, int RESUP>
__global__ void __launch_bounds__(256, (WM * WN <= 2 && BK == 32) ? 3 : 1)
conv_igemm_f32_kernel(const ConvParams p)
{
    constexpr int BN = WAVES_N * WN * 32;
    constexpr int BM = WAVES_M * WM * 32;
    constexpr int LDA = BM + 1;
    constexpr int CH4 = BK / 4;        // float4 channel groups per slab row (8 or 16)
    constexpr int RP = 256 / CH4;      // pixels staged per pass of the 256 threads (32 or 16)
    constexpr int PXT = BM / RP;       // pixels staged per thread per slab (2 or 4)
    constexpr int KS = BK / 2;
    static_assert((BM == 128 || BM == 64) && WAVES_M * WAVES_N == 4, "tile");
    static_assert(BN == 32 || BN == 64 || BN == 128, "BN");
    static_assert((BK == 32 || BK == 64) && PXT <= 4, "BK");
    constexpr int B_F4 = (BK * BN / 4) / 256;  // float4 per thread for the B slab (1, 2 or 4)
    constexpr int BROWS = 256 / (BN / 4);      // B slab rows covered by one pass of the 256 threads
    static_assert(B_F4 >= 1 && B_F4 <= 4, "B staging");
    constexpr bool MOD = DEFORM == 2;
    constexpr bool DEF = DEFORM == 1 || DEFORM == 2;
    constexpr bool STEM = DEFORM == 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *As = reinterpret_cast<float *>(smem_raw);     // [2][BK][LDA]
    float *Bs = As + 2 * BK * LDA;                       // [2][BK][BN]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;
    const int akr = lane >> 5, aij = lane & 31;
    // XCD-aware tile order. Workgroup b is observed to run on XCD b % 8 (speed only, never correctness). Each XCD gets
    // a CONTIGUOUS range of m-tiles (so the 3x3 / bilinear halos of vertically adjacent tiles hit the same 4 MiB L2)
    // and all n-tiles of an m-tile (they share the A panel) stay on that XCD.
    int m_t, n_t, kz;
    {
        const int nt = p.n_tiles;
        const int per = (p.m_tiles + 7) >> 3;
        const int base_grid = 8 * per * nt;
        kz = RESUP == 3 ? (int)blockIdx.x / base_grid : 0;   // split-K part of this workgroup
        const int bid = (int)blockIdx.x - kz * base_grid;
        const int q = bid >> 3;
        n_t = q % nt;
        const int local = q / nt;
        m_t = (bid & 7) * per + local;
        if (local >= per || m_t >= p.m_tiles) return;
    }
    int si = 0;
#pragma unroll
    for (int q = 1; q < CV_MAXSEG; ++q) if (q < p.nseg && m_t >= p.seg[q].tile_start) si = q;
    const ConvSeg sg = p.seg[si];
    const long p0 = (long)(m_t - sg.tile_start) * BM;
    const int n0 = n_t * BN;
    const int ntap = p.KH * p.KW;

    // ---- per-thread A staging geometry: PXT pixels (prow + RP r), channels 4*ch4..+3 of the slab
    const int ch4 = tid % CH4, prow = tid / CH4;
    int pix_n[4], pix_h[4], pix_w[4];
    long pix_p[4];
    const long HoWo = (long)sg.Ho * sg.Wo;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long pp = p0 + prow + RP * r;
        if (r < PXT && pp < sg.M) {
            const int n = (int)(pp / HoWo);
            const int rem = (int)(pp - (long)n * HoWo);
            pix_n[r] = n; pix_h[r] = (rem / sg.Wo) * p.stride - p.pad; pix_w[r] = (rem % sg.Wo) * p.stride - p.pad;
            pix_p[r] = pp;
        } else { pix_n[r] = -1; pix_h[r] = 0; pix_w[r] = 0; pix_p[r] = -1; }
    }
    const int nslabs_all = ntap * (p.Cin / BK);
    const int s_per = RESUP == 3 ? (nslabs_all + p.ksplit - 1) / p.ksplit : nslabs_all;
    const int s_begin = kz * s_per;
    const int nslabs = max(min(nslabs_all - s_begin, s_per), 0);   // slabs walked by this workgroup (split-K: its share)

    floatx16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Operand addressing: uniform 64-bit base + 32-bit per-lane byte offset (one global_load each, no 64-bit VALU).
    // Loads are UNCONDITIONAL (clamped addresses); zero-fill / validity is applied when the registers are written
    // to LDS -- a "load or 0" select at the load site makes hipcc branch around every load and wait vmcnt(0) each.
    // All staging state is in named scalars: arrays captured by lambdas / indexed in loops were demoted to scratch.
    const char *xbase = reinterpret_cast<const char *>(sg.x);
    const unsigned ldw4 = 4u * (unsigned)p.ldw;
    const unsigned cin4 = 4u * (unsigned)p.Cin, wcin4 = cin4 * (unsigned)sg.W;  // byte steps to the right / lower pixel
    const char *wb0 = reinterpret_cast<const char *>(sg.w != nullptr ? sg.w : p.w) + 4 * n0;
    const char *wb1 = wb0 + (size_t)BROWS * ldw4, *wb2 = wb0 + (size_t)2 * BROWS * ldw4, *wb3 = wb0 + (size_t)3 * BROWS * ldw4;
    unsigned ob = (unsigned)(tid / (BN / 4)) * ldw4 + 16u * (unsigned)(tid % (BN / 4));  // advances BK rows per slab
    unsigned oa0 = 0, oa1 = 0, oa2 = 0, oa3 = 0;               // dense: byte offset of this thread's float4 per pixel
    bool cv0 = false, cv1 = false, cv2 = false, cv3 = false;   // dense: tap inside the image
    int f_cs = 0, f_tap = 0, f_ki = 0, f_kj = 0;               // (channel slab, tap) of the NEXT slab to fetch
    if (RESUP == 3) {   // split-K: start the K walk at slab s_begin
        const int cslabs = p.Cin / BK;
        f_tap = s_begin / cslabs;
        f_cs = (s_begin - f_tap * cslabs) * BK;
        f_ki = f_tap / p.KW;
        f_kj = f_tap - f_ki * p.KW;
        ob += (unsigned)s_begin * (unsigned)BK * ldw4;
    }
    bool f_newtap = true;
    float4 xa0, xa1, xa2, xa3, xb0, xb1, xb2, xb3;             // dense register set X
    float4 ya0, ya1, ya2, ya3, yb0, yb1, yb2, yb3;             // dense register set Y
    bool xv0 = false, xv1 = false, xv2 = false, xv3 = false, yv0 = false, yv1 = false, yv2 = false, yv3 = false;
    float4 c00, c01, c02, c03, c10, c11, c12, c13, c20, c21, c22, c23, c30, c31, c32, c33;  // deformable: [pixel][corner]
    DcnDesc d0, d1, d2, d3;

#define CV_LDX(O) (*reinterpret_cast<const float4 *>(xbase + (O)))
#define CV_TAP_DENSE(R)                                                                                               \
    {                                                                                                                 \
        const int hi = pix_h[R] + f_ki * p.dil, wi = pix_w[R] + (STEM ? ch4 : f_kj * p.dil);                          \
        cv##R = pix_n[R] >= 0 && hi >= 0 && hi < sg.H && wi >= 0 && wi < sg.W;                                        \
        const int hc = min(max(hi, 0), sg.H - 1), wc = min(max(wi, 0), sg.W - 1), nc = max(pix_n[R], 0);             \
        oa##R = STEM ? 16u * (unsigned)((nc * sg.H + hc) * sg.W + wc)                                                 \
                     : 4u * (unsigned)(((nc * sg.H + hc) * sg.W + wc) * p.Cin + f_cs + 4 * ch4);                      \
    }
#define CV_TAP_DEFORM(R)                                                                                              \
    d##R = dcn_desc(sg, pix_p[R], max(pix_n[R], 0) * sg.H * sg.W * p.Cin + 4 * ch4, f_tap, ntap,                      \
                    pix_h[R] + f_ki * p.dil, pix_w[R] + f_kj * p.dil, p.Cin, MOD);
#define CV_ADVANCE                                                                                                    \
    ob += (unsigned)BK * ldw4;                                                                                        \
    f_cs += BK;                                                                                                       \
    f_newtap = f_cs == p.Cin;                                                                                         \
    if (f_newtap) { f_cs = 0; ++f_tap; if (++f_kj == p.KW) { f_kj = 0; ++f_ki; } }
#define CV_FETCH_B(P)                                                                                                 \
    P##b0 = *reinterpret_cast<const float4 *>(wb0 + ob);                                                              \
    if (B_F4 > 1) P##b1 = *reinterpret_cast<const float4 *>(wb1 + ob);                                                \
    if (B_F4 > 2) { P##b2 = *reinterpret_cast<const float4 *>(wb2 + ob); P##b3 = *reinterpret_cast<const float4 *>(wb3 + ob); }
#define CV_FETCH_DENSE(P)                                                                                             \
    {                                                                                                                 \
        if (f_newtap) { CV_TAP_DENSE(0) CV_TAP_DENSE(1) if (PXT > 2) { CV_TAP_DENSE(2) CV_TAP_DENSE(3) } }            \
        P##a0 = CV_LDX(oa0); P##v0 = cv0; oa0 += 4u * BK;                                                             \
        P##a1 = CV_LDX(oa1); P##v1 = cv1; oa1 += 4u * BK;                                                             \
        if (PXT > 2) {                                                                                                \
            P##a2 = CV_LDX(oa2); P##v2 = cv2; oa2 += 4u * BK;                                                         \
            P##a3 = CV_LDX(oa3); P##v3 = cv3; oa3 += 4u * BK;                                                         \
        }                                                                                                             \
        CV_FETCH_B(P)                                                                                                 \
        CV_ADVANCE                                                                                                    \
    }
#define CV_FETCH_DEFORM_PX(R)                                                                                         \
    {                                                                                                                 \
        const unsigned oR_ = d##R.o1 + ((d##R.vb & 16u) ? cin4 : 0u), oD_ = d##R.o1 + ((d##R.vb & 32u) ? wcin4 : 0u); \
        c##R##0 = CV_LDX(d##R.o1); c##R##1 = CV_LDX(oR_); c##R##2 = CV_LDX(oD_); c##R##3 = CV_LDX(oD_ + (oR_ - d##R.o1)); \
        d##R.o1 += 4u * BK;                                                                                           \
    }
#define CV_FETCH_DEFORM                                                                                               \
    {                                                                                                                 \
        if (f_newtap) { CV_TAP_DEFORM(0) CV_TAP_DEFORM(1) if (PXT > 2) { CV_TAP_DEFORM(2) CV_TAP_DEFORM(3) } }        \
        CV_FETCH_DEFORM_PX(0) CV_FETCH_DEFORM_PX(1)                                                                   \
        if (PXT > 2) { CV_FETCH_DEFORM_PX(2) CV_FETCH_DEFORM_PX(3) }                                                  \
        CV_FETCH_B(x)                                                                                                 \
        CV_ADVANCE                                                                                                    \
    }
#define CV_FETCH_x CV_FETCH_DENSE(x)
#define CV_FETCH_y CV_FETCH_DENSE(y)
#define CV_FETCH_c CV_FETCH_DEFORM
#define CV_FETCH(SET) CV_FETCH_##SET

#define CV_STASH_PX(BUF, R, VX, VY, VZ, VW)                                                                           \
    {                                                                                                                 \
        float *sa = As + (BUF) * BK * LDA + prow + RP * R;                                                            \
        sa[(4 * ch4 + 0) * LDA] = VX;                                                                                 \
        sa[(4 * ch4 + 1) * LDA] = VY;                                                                                 \
        sa[(4 * ch4 + 2) * LDA] = VZ;                                                                                 \
        sa[(4 * ch4 + 3) * LDA] = VW;                                                                                 \
    }
#define CV_STASH_A_DENSE(P, BUF, R)                                                                                   \
    CV_STASH_PX(BUF, R, P##v##R ? P##a##R.x : 0.f, P##v##R ? P##a##R.y : 0.f, P##v##R ? P##a##R.z : 0.f, P##v##R ? P##a##R.w : 0.f)
#define CV_STASH_A_x(BUF, R) CV_STASH_A_DENSE(x, BUF, R)
#define CV_STASH_A_y(BUF, R) CV_STASH_A_DENSE(y, BUF, R)
#define CV_STASH_A_c(BUF, R)                                                                                          \
    CV_STASH_PX(BUF, R, dcn_blend1(d##R, (c##R##0).x, (c##R##1).x, (c##R##2).x, (c##R##3).x, MOD),                            \
                dcn_blend1(d##R, (c##R##0).y, (c##R##1).y, (c##R##2).y, (c##R##3).y, MOD),                                    \
                dcn_blend1(d##R, (c##R##0).z, (c##R##1).z, (c##R##2).z, (c##R##3).z, MOD),                                    \
                dcn_blend1(d##R, (c##R##0).w, (c##R##1).w, (c##R##2).w, (c##R##3).w, MOD))
#define CV_STASH_A(SET, BUF, R) CV_STASH_A_##SET(BUF, R)
#define CV_STASH_B_P(P, BUF)                                                                                          \
    {                                                                                                                 \
        float4 *sb = reinterpret_cast<float4 *>(Bs + (BUF) * BK * BN);                                                \
        sb[tid] = P##b0;                                                                                              \
        if (B_F4 > 1) sb[tid + 256] = P##b1;                                                                          \
        if (B_F4 > 2) { sb[tid + 512] = P##b2; sb[tid + 768] = P##b3; }                                               \
    }
#define CV_STASH_B_x(BUF) CV_STASH_B_P(x, BUF)
#define CV_STASH_B_y(BUF) CV_STASH_B_P(y, BUF)
#define CV_STASH_B_c(BUF) CV_STASH_B_P(x, BUF)
#define CV_STASH_B(SET, BUF) CV_STASH_B_##SET(BUF)

    float av[2][WM], bv[2][WN];  // MFMA fragments, double-buffered over k steps (carried across slabs)
#define CV_FRAG(BUF, K, SLOT)                                                                                         \
    {                                                                                                                 \
        const float *a_ = As + (BUF) * BK * LDA + wm * (WM * 32) + aij + (2 * (K) + akr) * LDA;                       \
        const float *b_ = Bs + (BUF) * BK * BN + wn * (WN * 32) + aij + (2 * (K) + akr) * BN;                         \
        _Pragma("unroll") for (int i = 0; i < WM; ++i) av[SLOT][i] = a_[32 * i];                                      \
        _Pragma("unroll") for (int j = 0; j < WN; ++j) bv[SLOT][j] = b_[32 * j];                                      \
    }
// one slab: contract LDS buffer BUF; DO_FETCH: issue loads into FSET; DO_STASH: registers SSET -> buffer BUF^1
#define CV_SLAB(BUF, FSET, SSET, DO_FETCH, DO_STASH)                                                                  \
    {                                                                                                                 \
        const bool do_fetch_ = (DO_FETCH), do_stash_ = (DO_STASH);                                                    \
        _Pragma("unroll") for (int k = 0; k < KS; ++k) {                                                              \
            const int cur = k & 1, nxt = cur ^ 1;                                                                     \
            if (k == 0 && do_fetch_) CV_FETCH(FSET)                                                                   \
            if (k + 1 < KS) CV_FRAG(BUF, k + 1, nxt)                                                                  \
            else if (do_stash_) CV_FRAG((BUF) ^ 1, 0, nxt)                                                            \
            if (do_stash_) {                                                                                          \
                if (k == KS - 6) CV_STASH_A(SSET, (BUF) ^ 1, 0)                                                       \
                if (k == KS - 5) CV_STASH_A(SSET, (BUF) ^ 1, 1)                                                       \
                if (PXT > 2 && k == KS - 4) CV_STASH_A(SSET, (BUF) ^ 1, 2)                                            \
                if (PXT > 2 && k == KS - 3) CV_STASH_A(SSET, (BUF) ^ 1, 3)                                            \
                if (k == KS - 3) CV_STASH_B(SSET, (BUF) ^ 1)                                                          \
            }                                                                                                         \
            if (k == KS - 2) __syncthreads();                                                                         \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
            _Pragma("unroll") for (int i = 0; i < WM; ++i)                                                            \
                _Pragma("unroll") for (int j = 0; j < WN; ++j)                                                        \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[cur][i], bv[cur][j], acc[i][j], 0, 0, 0);     \
            __builtin_amdgcn_sched_barrier(0);                                                                        \
        }                                                                                                             \
    }

    if (DEF) {
        CV_FETCH(c)
        CV_STASH_A(c, 0, 0) CV_STASH_A(c, 0, 1)
        if (PXT > 2) { CV_STASH_A(c, 0, 2) CV_STASH_A(c, 0, 3) }
        CV_STASH_B(c, 0)
        __syncthreads();
        CV_FRAG(0, 0, 0)
        for (int s = 0; s < nslabs; s += 2) {
            CV_SLAB(0, c, c, s + 1 < nslabs, s + 1 < nslabs)
            if (s + 1 >= nslabs) break;
            CV_SLAB(1, c, c, s + 2 < nslabs, s + 2 < nslabs)
        }
    } else {
        CV_FETCH(x)
        CV_STASH_A(x, 0, 0) CV_STASH_A(x, 0, 1)
        if (PXT > 2) { CV_STASH_A(x, 0, 2) CV_STASH_A(x, 0, 3) }
        CV_STASH_B(x, 0)
        if (nslabs > 1) CV_FETCH(y)
        __syncthreads();
        CV_FRAG(0, 0, 0)
        for (int s = 0; s < nslabs; s += 2) {
            CV_SLAB(0, x, y, s + 2 < nslabs, s + 1 < nslabs)
            if (s + 1 >= nslabs) break;
            CV_SLAB(1, y, x, s + 3 < nslabs, s + 2 < nslabs)
        }
    }
#undef CV_LDX
#undef CV_TAP_DENSE
#undef CV_TAP_DEFORM
#undef CV_ADVANCE
#undef CV_FETCH_B
#undef CV_FETCH_DENSE
#undef CV_FETCH_DEFORM_PX
#undef CV_FETCH_DEFORM
#undef CV_FETCH_x
#undef CV_FETCH_y
#undef CV_FETCH_c
#undef CV_FETCH
#undef CV_STASH_PX
#undef CV_STASH_A_DENSE
#undef CV_STASH_A_x
#undef CV_STASH_A_y
#undef CV_STASH_A_c
#undef CV_STASH_A
#undef CV_STASH_B_P
#undef CV_STASH_B_x
#undef CV_STASH_B_y
#undef CV_STASH_B_c
#undef CV_STASH_B
#undef CV_FRAG
#undef CV_SLAB

    if (RESUP == 3) {
        // ---- split-K: raw partial sums to the workspace; bias / residual / ReLU are applied by conv_splitk_reduce_kernel
        if (nslabs <= 0) {
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        }
        float *part = p.partial + ((long)kz * p.m_total + (long)sg.tile_start * BM) * p.Cout;   // maps are concatenated tile-aligned
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                const int co = n0 + wn * (WN * 32) + 32 * j + aij;
                const long pbase = p0 + wm * (WM * 32) + 32 * i + 4 * akr;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long pp = pbase + (r & 3) + 8 * (r >> 2);
                    if (co < p.Cout && pp < sg.M) part[pp * p.Cout + co] = acc[i][j][r];
                }
            }
        return;
    }
    // ---- fused epilogue: + bias, + residual, ReLU. Residual values are loaded 16 at a time, unconditionally
    // (clamped row), before any of them is used, so the loads overlap instead of serialising.
    // RESUP 1: the residual lives at half resolution and is read through a nearest x2 upsampling
    //   (F.interpolate(scale_factor=2, mode='nearest') of the FPN top-down path, fpn.py:34,90-96): src = (h >> 1, w >> 1).
    // RESUP 2: transposed 2x2 / stride-2 convolution (mask head, rcnn.py:60,84): column co = (dy*2+dx)*C + c of output
    //   pixel (h, w) is channel c of output pixel (2h+dy, 2w+dx); bias is indexed by c.
    const bool has_res = sg.res != nullptr, has_bias = p.bias != nullptr;
    constexpr bool res_up = RESUP == 1, scatter = RESUP == 2;
    const int Hr = sg.Ho >> 1, Wr = sg.Wo >> 1;
    const int Cr = p.Cout >> 2;   // scatter: real output channels
    // r08: residual loads and stores through buffer descriptors with 32-bit byte offsets (no 64-bit index per element); an element
    // beyond the map / a padded column is an out-of-range offset: the load returns 0, the store is dropped.
    const unsigned crow = (unsigned)(scatter ? Cr : p.Cout) * 4u;       // bytes of one output pixel
    const size_t oaddr = reinterpret_cast<size_t>(sg.out);
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(oaddr >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)oaddr)),
        0, (int)__builtin_amdgcn_readfirstlane((unsigned)sg.M * (unsigned)p.Cout * 4u), 0x00020000);   // (scatter: 4 M pixels of Cout / 4 channels)
    const size_t raddr = reinterpret_cast<size_t>(has_res ? sg.res : sg.out);
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(raddr >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)raddr)),
        0, (int)__builtin_amdgcn_readfirstlane((unsigned)(res_up ? (long)sg.N * Hr * Wr : sg.M) * (unsigned)p.Cout * 4u), 0x00020000);
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        const long pbase = p0 + wm * (WM * 32) + 32 * i + 4 * akr;
        // pixel coordinates of this thread's 16 rows (only for the two coordinate-dependent epilogues): one division for the
        // first row; the other rows (offsets <= 27) are reached by increments with at most one line / image wrap when
        // Wo >= 32 (otherwise divide per row)
        unsigned ridx[16];      // res_up: half-resolution source pixel; scatter: top-left pixel of the 2x2 output block
        if (RESUP != 0) {
            const long pb = pbase < sg.M ? pbase : sg.M - 1;
            const int n_b = (int)(pb / HoWo);
            const int rem_b = (int)(pb - (long)n_b * HoWo);
            const int h_b = rem_b / sg.Wo, w_b = rem_b - h_b * sg.Wo;
            const bool fast = sg.Wo >= 32;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int off = (r & 3) + 8 * (r >> 2);
                int n = n_b, h = h_b, w = w_b;
                if (pbase + off < sg.M) {
                    if (fast) {
                        w += off;
                        if (w >= sg.Wo) { w -= sg.Wo; ++h; }
                        if (h >= sg.Ho) { h -= sg.Ho; ++n; }
                    } else {
                        const long pp = pbase + off;
                        n = (int)(pp / HoWo);
                        const int rem = (int)(pp - (long)n * HoWo);
                        h = rem / sg.Wo; w = rem - h * sg.Wo;
                    }
                }
                ridx[r] = res_up ? (unsigned)((n * Hr + (h >> 1)) * Wr + (w >> 1))
                                 : (unsigned)((n * 2 * sg.Ho + 2 * h) * (2 * sg.Wo) + 2 * w);
            }
        }
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            const int co = n0 + wn * (WN * 32) + 32 * j + aij;
            const bool co_ok = co < p.Cout;
            const int coc = co_ok ? co : 0;
            int cb = coc;          // bias / output channel
            unsigned soff = 0;     // scatter: byte offset of (dy, dx, channel) inside the 2x upsampled map
            if (scatter) {
                const int q = coc / Cr;
                cb = coc - q * Cr;
                soff = (unsigned)(((q >> 1) * (2 * sg.Wo) + (q & 1)) * Cr + cb) * 4u;
            }
            const float bv = has_bias ? p.bias[cb] : 0.f;
            float rr[16];
            if (has_res) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long pp = pbase + (r & 3) + 8 * (r >> 2);
                    const bool ok = co_ok && pp < sg.M;
                    const unsigned src = res_up ? ridx[r] : (unsigned)pp;
                    rr[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, ok ? src * ((unsigned)p.Cout * 4u) + 4u * (unsigned)co : 0x80000000u, 0, 0));
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long pp = pbase + (r & 3) + 8 * (r >> 2);
                float v = acc[i][j][r];
                if (has_bias) v = v + bv;
                if (has_res) v = v + rr[r];
                if (p.relu) v = fmaxf(v, 0.f);
                const bool ok = co_ok && pp < sg.M;
                const unsigned dst = scatter ? ridx[r] * crow + soff : (unsigned)pp * crow + 4u * (unsigned)co;
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orsrc, ok ? dst : 0x80000000u, 0, 0);
            }
        }
    }
}

template <int WM, int WN, int WAVES_M, int WAVES_N, int DEFORM, int BK = CV_BK, int RESUP = 0>
static int conv_launch(hipStream_t st, ConvParams &p)
{
    constexpr int BN = WAVES_N * WN * 32, BM = WAVES_M * WM * 32;
    // re-tile the feature maps for this BM
    int tiles = 0;
    for (int i = 0; i < p.nseg; ++i) { p.seg[i].tile_start = tiles; tiles += (int)((p.seg[i].M + BM - 1) / BM); }
    p.m_tiles = tiles;
    p.n_tiles = (p.Cout + BN - 1) / BN;
    const size_t smem = (size_t)(2 * BK * (BM + 1) + 2 * BK * BN) * sizeof(float);
    static std::atomic<unsigned long long> attr_dev{0};  // > 64 KiB of dynamic LDS must be opted into once per kernel
    if (smem > 64 * 1024)
        UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_igemm_f32_kernel<WM, WN, WAVES_M, WAVES_N, DEFORM, BK, RESUP>),
                                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)));
    p.m_total = (long)p.m_tiles * BM;
    const int grid = 8 * ((p.m_tiles + 7) / 8) * p.n_tiles * (RESUP == 3 ? p.ksplit : 1);  // see the XCD-aware tile order in the kernel
    hipLaunchKernelGGL((conv_igemm_f32_kernel<WM, WN, WAVES_M, WAVES_N, DEFORM, BK, RESUP>), dim3(grid), dim3(256), smem, st, p);
    UPS_CHECK_LAUNCH("conv_igemm_f32_kernel");
    return 0;
}

// Tile choice (measured on MI355X over every conv shape of UPSNet-50 @1024x2048, tools/sweep_conv_tiles.py): with the pinned
// schedule above one wave keeps the MFMA pipe ~80 % busy, and the 64x64 tile (107 registers, 33 KiB LDS -> 4 workgroups per
// CU) wins on every dense layer, from 2048 to 174592 pixels. The deformable variants use 64x128 (the A operand is an
// expensive gather, computed once per 128 output channels; 168 registers -> 3 waves per SIMD). Cout <= 32 heads use 128x32.
// upsnet_conv_tuning(0, force_tile) overrides for A/B runs.
static int g_force_tile = 0;
extern int g_wino_tm;
extern "C" void upsnet_conv_tuning(int winograd_tiles, int force_tile) { g_wino_tm = winograd_tiles; g_force_tile = force_tile; }

// Residency table (residency.h): workgroups per CU each multi-workgroup-per-CU kernel is held to by its launcher. All 0 = the launches
// as they always were. g_res_default: the caps the model turns on while it captures the graphs of two or more images in flight --
// chosen by end-to-end measurement, family by family (profiles/residency_sweep.txt); a family that did not win
// stays at 0. Only the 32-pixel pair kernel won: one workgroup per CU, +1.0 % (its 256 workgroups at 1024x2048 are one per CU).
int g_res_cap[RES_NKERNELS] = {0, 0, 0, 0, 0, 0, 0};
static const int g_res_default[RES_NKERNELS] = {0, 0, 1, 0, 0, 0, 0};   // indexed by ResKernel
extern "C" int upsnet_residency_tuning(int kernel, int cap)
{
    UPS_REQUIRE(kernel >= -1 && kernel < RES_NKERNELS, "residency_tuning: kernel must be -1 (all) or 0..%d", RES_NKERNELS - 1);
    UPS_REQUIRE(cap >= -1 && cap <= RES_MAX_CAP, "residency_tuning: cap must be -1 (the measured default), 0 (off) or 1..%d", RES_MAX_CAP);
    for (int k = 0; k < RES_NKERNELS; ++k)
        if (kernel < 0 || kernel == k) g_res_cap[k] = cap < 0 ? g_res_default[k] : cap;
    return 0;
}
int g_res_last_dynamic = 0;
extern "C" int upsnet_residency_last_dynamic_lds(void) { return g_res_last_dynamic; }
extern "C" size_t upsnet_residency_pad_bytes(int cap, size_t static_lds, size_t dynamic_lds) { return res_pad_bytes(cap, static_lds, dynamic_lds); }

template <int DEFORM>
static int conv_dispatch(hipStream_t st, ConvParams &p)
{
    const bool n128 = p.ldw % 128 == 0, n64 = p.ldw % 64 == 0;
    int tile = g_force_tile;
    if (!tile) {
        if (DEFORM) tile = n128 ? 4 : (n64 ? 5 : 3);
        else tile = n64 ? 5 : 3;
    }
    if (tile == 1 && !n128) tile = n64 ? 2 : 3;
    if ((tile == 2 || tile == 5) && !n64) tile = 3;
    if (tile == 4 && !n128) tile = n64 ? 5 : 3;
    if (tile == 6 && (!n64 || p.Cin % 64 != 0)) tile = n64 ? 5 : 3;
    if (p.res_up) {  // coordinate-dependent epilogues (FPN top-down add, deconvolution scatter): separate instances, dense only
        UPS_REQUIRE(DEFORM == 0, "conv: this epilogue is only available for dense convolution");
        if (p.res_up == 1) return n64 ? conv_launch<1, 1, 2, 2, 0, CV_BK, 1>(st, p) : conv_launch<1, 1, 4, 1, 0, CV_BK, 1>(st, p);
        return n64 ? conv_launch<1, 1, 2, 2, 0, CV_BK, 2>(st, p) : conv_launch<1, 1, 4, 1, 0, CV_BK, 2>(st, p);
    }
    if (p.ksplit > 1) {   // split-K instances (dense): partial sums to the workspace. 64x64 tile; 128x32 for the narrow heads (ldw = 32:
                          // the 18-channel offset predictors of the deformable bottlenecks on small maps, r10)
        UPS_REQUIRE(DEFORM == 0, "conv: split-K needs a dense convolution");
        return n64 ? conv_launch<1, 1, 2, 2, 0, CV_BK, 3>(st, p) : conv_launch<1, 1, 4, 1, 0, CV_BK, 3>(st, p);
    }
    if (DEFORM == 3) return n64 ? conv_launch<1, 1, 2, 2, 3>(st, p) : conv_launch<1, 1, 4, 1, 3>(st, p);
    constexpr int D = DEFORM >= 3 ? 0 : DEFORM;  // (the stem returned above; keeps its instantiations to two tiles)
    switch (tile) {
    case 1: return conv_launch<2, 2, 2, 2, D>(st, p);      // 128 x 128
    case 2: return conv_launch<1, 2, 4, 1, D>(st, p);      // 128 x 64
    case 4: return conv_launch<1, 2, 2, 2, D>(st, p);      // 64 x 128
    case 5: return conv_launch<1, 1, 2, 2, D>(st, p);      // 64 x 64
    case 6: return conv_launch<1, 1, 2, 2, D, 64>(st, p);  // 64 x 64, 64-channel K slabs
    default: return conv_launch<1, 1, 4, 1, D>(st, p);     // 128 x 32
    }
}

extern "C" int upsnet_conv2d_nhwc_f32(void *stream, int nseg, const float *const x[], const float *const residual[],
                                      float *const out[], const int batch[], const int height[], const int width[], int Cin,
                                      const float *wpack, int ldw, const float *bias, int Cout, int KH, int KW, int stride,
                                      int pad, int relu, int residual_up)
{
    ConvParams p;
    int rc = conv_fill(p, "conv2d_nhwc_f32", nseg, x, residual, nullptr, nullptr, out, batch, height, width, Cin, Cout, wpack, ldw,
                       bias, KH, KW, stride, pad, 1, relu);
    if (rc) return rc;
    if (residual_up) {
        UPS_REQUIRE(residual, "conv2d_nhwc_f32: residual_up without a residual");
        for (int i = 0; i < nseg; ++i)
            UPS_REQUIRE(p.seg[i].Ho % 2 == 0 && p.seg[i].Wo % 2 == 0, "conv2d_nhwc_f32: residual_up needs even output dims (map %d: %dx%d)", i, p.seg[i].Ho, p.seg[i].Wo);
        p.res_up = 1;
    }
    return conv_dispatch<0>((hipStream_t)stream, p);
}

/* The same geometry applied to several maps, each with ITS OWN packed weights, in one launch (no bias / residual): the per-level
 * column blocks of the FCN head's commuted 1x1 score (fcn.py:101-104: conv1x1(cat(up(y_l))) = sum_l up(W_l y_l)) -- four ~10 us launches
 * of 19 output channels are latency, not work. Every output is computed exactly as by upsnet_conv2d_nhwc_f32 on that map alone. */
extern "C" int upsnet_conv2d_nhwc_f32_multiw(void *stream, int nseg, const float *const x[], float *const out[], const int batch[],
                                             const int height[], const int width[], int Cin, const float *const wpack[], int ldw, int Cout,
                                             int KH, int KW, int stride, int pad, int relu)
{
    UPS_REQUIRE(wpack, "conv2d_nhwc_f32_multiw: null weight array");
    for (int i = 0; i < nseg && i < CV_MAXSEG; ++i) UPS_REQUIRE(wpack[i], "conv2d_nhwc_f32_multiw: null weights for map %d", i);
    ConvParams p;
    int rc = conv_fill(p, "conv2d_nhwc_f32_multiw", nseg, x, nullptr, nullptr, nullptr, out, batch, height, width, Cin, Cout, wpack[0], ldw,
                       nullptr, KH, KW, stride, pad, 1, relu);
    if (rc) return rc;
    for (int i = 0; i < nseg; ++i) p.seg[i].w = wpack[i];
    return conv_dispatch<0>((hipStream_t)stream, p);
}

extern "C" int upsnet_deform_conv_forward_nhwc(void *stream, int nlev, const float *const x[], const float *const offset[],
                                               const float *const mask[], float *const out[], const int height[],
                                               const int width[], int cin, int cout, int kh, int kw, int pad_h, int pad_w,
                                               int stride_h, int stride_w, int dil_h, int dil_w, int deformable_group,
                                               const float *wpack, int ldw, const float *bias, int relu)
{
    UPS_REQUIRE(deformable_group == 1, "deform_conv_forward_nhwc: deformable_group=%d not supported by the fused kernel (use the im2col path)", deformable_group);
    UPS_REQUIRE(pad_h == pad_w && stride_h == stride_w && dil_h == dil_w, "deform_conv_forward_nhwc: square stride/pad/dilation only");
    UPS_REQUIRE(nlev >= 1 && nlev <= 4 && offset, "deform_conv_forward_nhwc: nlev must be 1..4 and offsets given");
    for (int l = 0; l < nlev; ++l) UPS_REQUIRE(offset[l] && (!mask || mask[l]), "deform_conv_forward_nhwc: null offset/mask at level %d", l);
    ConvParams p;
    int rc = conv_fill(p, "deform_conv_forward_nhwc", nlev, x, nullptr, offset, mask, out, nullptr, height, width, cin, cout, wpack,
                       ldw, bias, kh, kw, stride_h, pad_h, dil_h, relu);
    if (rc) return rc;
    return mask ? conv_dispatch<2>((hipStream_t)stream, p) : conv_dispatch<1>((hipStream_t)stream, p);
}

// the same reduction one element per thread, for channel counts that are not a multiple of 4 (Cout = 18 offset predictors)
__global__ void __launch_bounds__(256)
conv_splitk_reduce1_kernel(const float *__restrict__ partial, const int ksplit, const long m_total, const long M, const int Cout,
                           const float *__restrict__ bias, const float *__restrict__ res, const int relu, float *__restrict__ out)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * Cout) return;
    const int c = (int)(idx % Cout);
    float a = partial[idx];
    for (int z = 1; z < ksplit; ++z) a = a + partial[(long)z * m_total * Cout + idx];   // fixed order: bit-repeatable
    if (bias) a = a + bias[c];
    if (res) a = a + res[idx];
    if (relu) a = fmaxf(a, 0.f);
    out[idx] = a;
}

// split-K reduction + the fused epilogue: out = relu?(sum_z partial[z] + bias + residual), float4 along the channels
__global__ void __launch_bounds__(256)
conv_splitk_reduce_kernel(const float *__restrict__ partial, const int ksplit, const long m_total, const long M, const int Cout,
                          const float *__restrict__ bias, const float *__restrict__ res, const int relu, float *__restrict__ out)
{
    const int c4n = Cout >> 2;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * c4n) return;
    const long pp = idx / c4n;
    const int c4 = (int)(idx - pp * c4n);
    float4 a = reinterpret_cast<const float4 *>(partial + pp * Cout)[c4];
    for (int z = 1; z < ksplit; ++z) {   // fixed order: bit-repeatable
        const float4 b = reinterpret_cast<const float4 *>(partial + ((long)z * m_total + pp) * Cout)[c4];
        a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w;
    }
    if (bias) { const float4 b = reinterpret_cast<const float4 *>(bias)[c4]; a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w; }
    if (res) { const float4 b = reinterpret_cast<const float4 *>(res + pp * Cout)[c4]; a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w; }
    if (relu) { a.x = fmaxf(a.x, 0.f); a.y = fmaxf(a.y, 0.f); a.z = fmaxf(a.z, 0.f); a.w = fmaxf(a.w, 0.f); }
    reinterpret_cast<float4 *>(out + pp * Cout)[c4] = a;
}

int conv_splitk_reduce(hipStream_t st, const float *partial, int ksplit, long m_total, long M, int Cout, const float *bias, const float *res,
                       int relu, float *out)
{
    if (Cout % 4) {
        const long n1 = M * Cout;
        hipLaunchKernelGGL(conv_splitk_reduce1_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, partial, ksplit, m_total, M, Cout, bias,
                           res, relu, out);
        UPS_CHECK_LAUNCH("conv_splitk_reduce1_kernel");
        return 0;
    }
    const long n = M * (Cout / 4);
    hipLaunchKernelGGL(conv_splitk_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, partial, ksplit, m_total, M, Cout, bias,
                       res, relu, out);
    UPS_CHECK_LAUNCH("conv_splitk_reduce_kernel");
    return 0;
}

extern "C" size_t upsnet_conv2d_splitk_workspace_bytes(int batch, int height, int width, int Cout, int KH, int KW, int stride, int pad,
                                                       int ksplit)
{
    if (batch < 1 || height < 1 || width < 1 || Cout < 1 || KH < 1 || KW < 1 || stride < 1 || pad < 0 || ksplit < 1) return 0;
    const long Ho = ((long)height + 2L * pad - KH) / stride + 1, Wo = ((long)width + 2L * pad - KW) / stride + 1;   // widened first
    if (Ho <= 0 || Wo <= 0) return 0;
    const long M = (long)batch * Ho * Wo;
    const long m_pad = (M + 127) / 128 * 128;   // (tile-aligned for both split-K instances: 64- and 128-pixel tiles)
    return (size_t)ksplit * m_pad * Cout * sizeof(float);
}

extern "C" int upsnet_conv2d_nhwc_f32_splitk(void *stream, const float *x, const float *residual, float *out, int batch, int height, int width,
                                             int Cin, const float *wpack, int ldw, const float *bias, int Cout, int KH, int KW, int stride,
                                             int pad, int relu, int ksplit, void *workspace)
{
    const float *xs[1] = {x}, *rs[1] = {residual};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    int rc = conv_fill(p, "conv2d_nhwc_f32_splitk", 1, xs, residual ? rs : nullptr, nullptr, nullptr, os, nb, hh, ww, Cin, Cout, wpack, ldw,
                       bias, KH, KW, stride, pad, 1, relu);
    if (rc) return rc;
    const int nslabs = KH * KW * (Cin / CV_BK);
    UPS_REQUIRE(workspace && ksplit >= 2 && ksplit <= 8, "conv2d_nhwc_f32_splitk: ksplit must be 2..8 and a workspace given");
    UPS_REQUIRE(((nslabs + ksplit - 1) / ksplit) * (ksplit - 1) < nslabs, "conv2d_nhwc_f32_splitk: %d K slabs cannot be split %d ways", nslabs, ksplit);
    p.ksplit = ksplit;
    p.partial = (float *)workspace;
    rc = conv_dispatch<0>((hipStream_t)stream, p);
    if (rc) return rc;
    return conv_splitk_reduce((hipStream_t)stream, p.partial, ksplit, p.m_total, p.seg[0].M, Cout, bias, residual, relu, out);
}


extern "C" int upsnet_conv2d_stem_nhwc4_f32(void *stream, const float *x, int batch, int height, int width, const float *wpack,
                                            int ldw, const float *bias, int Cout, int KH, int KW, int stride, int pad, int relu,
                                            float *out)
{
    UPS_REQUIRE(KW >= 1 && KW <= 8, "conv2d_stem_nhwc4_f32: kernel width must be <= 8 (got %d)", KW);
    const float *xs[1] = {x};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    // geometry from the real kernel; the K walk sees KH taps of 32 "channels" (8 pixels x 4 channels of one kernel row)
    int rc = conv_fill(p, "conv2d_stem_nhwc4_f32", 1, xs, nullptr, nullptr, nullptr, os, nb, hh, ww, 32, Cout, wpack, ldw, bias, KH, KW,
                       stride, pad, 1, relu);
    if (rc) return rc;
    p.KW = 1;
    return conv_dispatch<3>((hipStream_t)stream, p);
}

extern "C" int upsnet_deconv2x2_nhwc_f32(void *stream, const float *x, int batch, int height, int width, int Cin, const float *wpack,
                                         int ldw, const float *bias, int Cout, int relu, float *out)
{
    UPS_REQUIRE(Cout > 0 && ldw >= 4 * Cout, "deconv2x2_nhwc_f32: ldw must cover 4*Cout columns");
    const float *xs[1] = {x};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    int rc = conv_fill(p, "deconv2x2_nhwc_f32", 1, xs, nullptr, nullptr, nullptr, os, nb, hh, ww, Cin, 4 * Cout, wpack, ldw, bias, 1, 1, 1, 0,
                       1, relu);
    if (rc) return rc;
    UPS_REQUIRE((long)batch * height * width * 4 * Cout < (1L << 31), "deconv2x2_nhwc_f32: output too large");
    p.res_up = 2;
    return conv_dispatch<0>((hipStream_t)stream, p);
}

// stem: weight [Cout, Cin<=4, KH, KW<=8] -> wpack [(ki*32 + kj*4 + c), ldw]; deconv: weight [Cin, Cout, 2, 2] ->
// wpack [ci, (dy*2+dx)*Cout + co]; zero padded
__global__ void conv_pack_weight_stem_kernel(const float *__restrict__ w, int cout, int cin, int kh, int kw, int ldw, float *__restrict__ wp)
{
    const long total = (long)ldw * 32 * kh;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)blockDim.x * gridDim.x) {
        const int co = idx % ldw;
        const int k = (idx / ldw) % 32, ki = idx / ((long)ldw * 32);
        const int kj = k >> 2, c = k & 3;
        wp[idx] = (co < cout && c < cin && kj < kw) ? w[(((long)co * cin + c) * kh + ki) * kw + kj] : 0.f;
    }
}

__global__ void deconv2x2_pack_weight_kernel(const float *__restrict__ w, int cin, int cout, int ldw, float *__restrict__ wp)
{
    const long total = (long)ldw * cin;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)blockDim.x * gridDim.x) {
        const int col = idx % ldw, ci = idx / ldw;
        const int q = col / cout, co = col - q * cout;
        wp[idx] = q < 4 ? w[((long)ci * cout + co) * 4 + q] : 0.f;
    }
}

extern "C" int upsnet_conv_pack_weight_stem(void *stream, const float *weight, int cout, int cin, int kh, int kw, int ldw, float *wpack)
{
    UPS_REQUIRE(weight && wpack && cout > 0 && cin >= 1 && cin <= 4 && kh >= 1 && kw >= 1 && kw <= 8 && ldw >= cout && ldw % 32 == 0,
                "conv_pack_weight_stem: bad args (Cin <= 4, KW <= 8)");
    const long total = (long)ldw * 32 * kh;
    hipLaunchKernelGGL(conv_pack_weight_stem_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, weight,
                       cout, cin, kh, kw, ldw, wpack);
    UPS_CHECK_LAUNCH("conv_pack_weight_stem_kernel");
    return 0;
}

extern "C" int upsnet_deconv2x2_pack_weight(void *stream, const float *weight, int cin, int cout, int ldw, float *wpack)
{
    UPS_REQUIRE(weight && wpack && cin > 0 && cout > 0 && ldw >= 4 * cout && ldw % 32 == 0, "deconv2x2_pack_weight: bad args");
    const long total = (long)ldw * cin;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(deconv2x2_pack_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, cin, cout, ldw, wpack);
    UPS_CHECK_LAUNCH("deconv2x2_pack_weight_kernel");
    return 0;
}

// weight [Cout, Cin, kh, kw] -> wpack [(tap*Cin + c), ldw], zero padded columns
__global__ void conv_pack_weight_kernel(const float *__restrict__ w, int cout, int cin, int taps, int ldw, float *__restrict__ wp)
{
    const long total = (long)ldw * cin * taps;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)blockDim.x * gridDim.x) {
        const int co = idx % ldw;
        const int c = (idx / ldw) % cin;
        const int tap = idx / ((long)ldw * cin);
        wp[idx] = co < cout ? w[((long)co * cin + c) * taps + tap] : 0.f;
    }
}

extern "C" int upsnet_conv_pack_weight(void *stream, const float *weight, int cout, int cin, int kh, int kw, int ldw, float *wpack)
{
    UPS_REQUIRE(weight && wpack && cout > 0 && cin > 0 && kh > 0 && kw > 0 && ldw >= cout, "conv_pack_weight: bad args");
    const long total = (long)ldw * cin * kh * kw;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(conv_pack_weight_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, cout, cin, kh * kw, ldw, wpack);
    UPS_CHECK_LAUNCH("conv_pack_weight_kernel");
    return 0;
}
