// conv_wino.hip -- Winograd F(2x2, 3x3) convolution, fp32 MFMA, NHWC, all 16 transform-domain accumulators resident.
//
// Replaces the 3x3 / stride 1 / pad 1 nn.Conv2d (+ folded BN, bias, residual, ReLU) layers of the reference's ResNet-FPN
// (upsnet/models/resnet.py:64-77, fpn.py:60-98, rpn.py:34-47), of the mask head (rcnn.py:96-116) and the offset convolutions of
// the deformable FCN head (fcn.py:33-60) where the feature map has enough 2x2 tiles (models/hipconv.py decides by shape).
//
// GEMM view: a row is one 2x2 OUTPUT TILE (its 4x4 input patch d), a column one output channel; for each of the 16 positions
// xi = (i, j) of the transformed domain M_xi = V_xi x U_xi with V = B^T d B (input transform) and U = G g G^T (weights, packed
// once). In the base form a workgroup (8 waves, two per SIMD) owns 64 tiles x 64 channels and keeps ALL 16 M_xi accumulators in
// registers (the 32-tile / 32-channel forms are described at the kernel template):
// wave (pair, xh) holds the 32x32 block `pair` of the eight M_xi with xi in [8 xh, 8 xh + 8) = 128 accumulator registers, so
//   * the K walk over the input channels happens ONCE: every input pixel of the patch is loaded once per slab and transformed
//     once (the earlier form walked K once per xi and gathered four signed pixels per A element: 4x the loads, 16x the walks),
//   * the two waves of a SIMD cover each other: while one runs its chain of dependent MFMAs the other issues the loads, the
//     transform and the LDS traffic (a single wave per SIMD left ~20 % of the MFMA pipe idle behind them),
//   * the output transform Y = A^T M A needs one exchange between the two waves of a pair (M_1j <-> M_2j through LDS), after
//     which wave xh computes and stores output row xh of every 2x2 tile.
// Per slab of 16 input channels: thread (tile, channel pair c2) loads the tile's 16 patch pixels (float2; out-of-image pixels
// read as 0 through the buffer bounds check), transforms them (32 float2 adds) and writes V_xi to LDS as 16-byte units
// [xi][q = c2/2][tile ^ 2q] -- conflict-free for the ds_write_b64 and for the fragment ds_read_b128 (lane = (row, k-half)
// reads unit [xi][2h + half][row ^ (4h + 2 half)]: 16 distinct slots per lane group). The MFMA is v_mfma_f32_32x32x2_f32:
// lane l supplies A[row l%32][k l/32], so a float4 fragment feeds four MFMAs (lanes < 32 walk quarter 2h, lanes >= 32 quarter
// 2h+1). The B operand (U) does not go through LDS: it is packed as [n-tile][slab][xi][q][64 channels][4] so that a lane's
// fragment is one 16-byte load, contiguous across the wave (1 KiB), prefetched in a register ring.
// LDS: 2 buffers x 64 KiB (double-buffered V), one workgroup per CU; the 32-tile forms: 2 x 32 KiB, two workgroups per CU.
#include <cstdlib>
#include "conv_params.h"
#include "residency.h"
#include "upsnet_hip.h"

#define WG_STEPS 32          // (xi, h) steps per slab: 16 positions x 2 k-halves of 8 channels; 16 per wave

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));
typedef unsigned uintx2 __attribute__((ext_vector_type(2)));

// The input transform runs beside the MFMAs of the K loop. Written as plain float2 arithmetic the compiler forms v_pk_add_f32,
// and a packed fp32 VALU instruction next to MFMAs costs far more than its issue slot (MI355X guide: ~+13 cycles each); the
// scalar v_add_f32 / v_sub_f32 hide in the MFMA shadow. Same IEEE operations, so the results are bit-identical.
__device__ static inline float f1sub(const float a, const float b) { float r; asm("v_sub_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ static inline float f1add(const float a, const float b) { float r; asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ static inline float2 f2sub(const float2 a, const float2 b) { return make_float2(f1sub(a.x, b.x), f1sub(a.y, b.y)); }
__device__ static inline float2 f2add(const float2 a, const float2 b) { return make_float2(f1add(a.x, b.x), f1add(a.y, b.y)); }

// SPLITK: the K walk is divided over p.ksplit workgroups per tile; each writes its raw output-transformed partial sums to
// p.partial [ksplit][N*OH*OW][Cout] (the transform is linear), reduced with bias / residual / ReLU by conv_splitk_reduce_kernel.
// TM: 2x2 tiles per workgroup. 64: 8 waves (2 x 2 blocks x 2 position halves), one workgroup per CU. 32: 4 waves (1 x 2 blocks x
// 2 halves), two workgroups per CU -- the prologue / epilogue of one overlaps the K walk of the other and mid-size maps get
// twice the workgroups, for twice the B traffic per output.
// TN: output channels per workgroup. 64, or 32 (only with TM = 32) for the narrow heads (the DCN offset convolutions, Cout = 18,
// would waste 46 of 64 columns): one 32x32 block, the 16 positions split over FOUR waves (4 accumulators each).
template <bool SPLITK, int TM, int TN>
__device__ __forceinline__ void conv_wino16_body(const ConvParams &p, const int wg)
{
    static_assert(TN == 64 || (TN == 32 && TM == 32), "tile forms: 64x64, 32x64, 32x32");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    constexpr unsigned WG_BUF = 16u * 4u * TM * 16u;     // bytes of one V buffer: 16 xi x 4 q x TM tiles x 16 B
    constexpr int NPAIR = (TM / 32) * (TN / 32);         // 32x32 blocks of the workgroup tile
    constexpr int NX = (TM / 8) / NPAIR;                 // groups the 16 positions are split into (waves per block): 2 or 4
    constexpr int NA = 16 / NX;                          // accumulators (positions) per wave
    constexpr int NS = 2 * NA;                           // (xi, h) steps per wave and slab
    constexpr unsigned BSTEP = TN * 32u;                 // bytes of one step of the packed weights: 2 q x TN channels x 16 B
    constexpr int WG_RING = 4;                           // B fragments in flight per wave
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pair = wave % NPAIR, xh = wave / NPAIR;
    const int wm = TM == 64 ? (pair & 1) : 0, wn = TM == 64 ? (pair >> 1) : pair;
    const int lhalf = lane >> 5, l32 = lane & 31;
    // XCD-aware tile order (workgroup b runs on XCD b % 8): each XCD gets a contiguous range of m-tiles, and all n-tiles of an
    // m-tile (they share the input patches) stay on that XCD. Same scheme as conv_igemm_f32_kernel.
    int m_t, n_t, kz;
    {
        const int nt = p.n_tiles;
        const int per = (p.m_tiles + 7) >> 3;
        const int base_grid = 8 * per * nt;
        kz = SPLITK ? wg / base_grid : 0;
        const int bid = wg - kz * base_grid;
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
    const long p0 = (long)(m_t - sg.tile_start) * TM;
    const int n0 = n_t * TN;
    const int nslabs = p.Cin >> 4;
    const int s_per = SPLITK ? (nslabs + p.ksplit - 1) / p.ksplit : nslabs;
    const int s_begin = kz * s_per, s_end = min(s_begin + s_per, nslabs);   // slabs walked by this workgroup (launcher: never empty)
    const long HoWo = (long)sg.Ho * sg.Wo;       // tiles per image (Ho, Wo count 2x2 output tiles here)

    // ---- loader geometry: thread = (tile tid/8, channel pair tid%8)
    const int ltile = tid >> 3, lc2 = tid & 7, lq = lc2 >> 1;
    // byte offsets of the patch rows / columns for this thread's channel pair; a row or column outside the image carries a flag
    // bit that pushes the sum beyond the feature map (< 1 GiB, checked at launch), where the buffer load returns 0
    unsigned ro0, ro1, ro2, ro3, co0, co1, co2, co3;
    {
        const long pp = p0 + ltile;
        const bool tile_ok = pp < sg.M;
        const long ppc = tile_ok ? pp : sg.M - 1;
        const int n = (int)(ppc / HoWo);
        const int rem = (int)(ppc - (long)n * HoWo);
        const int ty = rem / sg.Wo, tx = rem - ty * sg.Wo;
        const int h0 = 2 * ty - 1, w0 = 2 * tx - 1;
        const unsigned cin4 = 4u * (unsigned)p.Cin;
        unsigned ro[4], co[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int h = h0 + r, w = w0 + r;
            const unsigned rv = (unsigned)((n * sg.H + min(max(h, 0), sg.H - 1)) * sg.W) * cin4;
            const unsigned cv = (unsigned)min(max(w, 0), sg.W - 1) * cin4 + 8u * (unsigned)lc2;
            ro[r] = rv | ((tile_ok && h >= 0 && h < sg.H) ? 0u : 0x80000000u);
            co[r] = cv | ((w >= 0 && w < sg.W) ? 0u : 0x40000000u);
        }
        ro0 = ro[0]; ro1 = ro[1]; ro2 = ro[2]; ro3 = ro[3];
        co0 = co[0]; co1 = co[1]; co2 = co[2]; co3 = co[3];
    }
    // buffer descriptors from provably uniform scalars (readfirstlane), so that no load is waterfalled
    const size_t xaddr = reinterpret_cast<size_t>(sg.x);
    const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr), xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
    const unsigned xbytes = __builtin_amdgcn_readfirstlane((unsigned)(sg.N * sg.H * sg.W) * 4u * (unsigned)p.Cin);
    const char *xbase = reinterpret_cast<const char *>(((size_t)xhi << 32) | xlo);
    // LDS addresses (bytes within a buffer): stash unit [xi][lq][ltile ^ 2 lq] (+ 4 planes per xi), this thread's 8-byte half;
    // fragment unit [2t + lhalf][row ^ (4h + 2 lhalf)] (+ 2 planes per step t), row = 32 wm + l32
    const unsigned st_base = (unsigned)((lq * TM + (ltile ^ (2 * lq))) * 16 + (lc2 & 1) * 8);
    const int frow = 32 * wm + l32;
    constexpr unsigned PLANE = TM * 16u;                  // bytes of one (xi, q) plane; a step t = (xi, h) spans two planes
    const unsigned fr_base0 = (unsigned)(lhalf * PLANE + (frow ^ (2 * lhalf)) * 16 + xh * NS * 2 * PLANE);
    const unsigned fr_base1 = (unsigned)(lhalf * PLANE + (frow ^ (4 + 2 * lhalf)) * 16 + xh * NS * 2 * PLANE);
    // B: lane's float4 of step g = slab * 32 + t sits at wbase + g * 2048 + lhalf * 1024 + (32 wn + l32) * 16
    const size_t waddr = reinterpret_cast<size_t>(p.w) + (size_t)n_t * (size_t)nslabs * (WG_STEPS * BSTEP);
    const unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)waddr), whi = __builtin_amdgcn_readfirstlane((unsigned)(waddr >> 32));
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)whi << 32) | wlo), 0,
                                                                            nslabs * (int)(WG_STEPS * BSTEP), 0x00020000);
    const unsigned b_lane = (unsigned)(lhalf * (TN * 16) + (32 * wn + l32) * 16);
    const int gmax = nslabs * WG_STEPS - 1;
    const int xh_u = __builtin_amdgcn_readfirstlane(xh);

    floatx16 acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

#define WG_PO(PX) (((PX) >> 2) == 0 ? ro0 : ((PX) >> 2) == 1 ? ro1 : ((PX) >> 2) == 2 ? ro2 : ro3) + (((PX) & 3) == 0 ? co0 : ((PX) & 3) == 1 ? co1 : ((PX) & 3) == 2 ? co2 : co3)
    float2 ld[16];     // patch pixels of the slab being staged; after the row pass: (d B)[r][j]
    float4 breg[WG_RING];

#define WG_LOAD(PX, RS) { const uintx2 v_ = __builtin_amdgcn_raw_buffer_load_b64(RS, WG_PO(PX), 0, 0); ld[PX] = make_float2(__uint_as_float(v_.x), __uint_as_float(v_.y)); }
    // row pass of the input transform on patch row R: (d B)[R][0..3]
#define WG_ROWPASS(R)                                                                                                 \
    {                                                                                                                 \
        const float2 d0 = ld[4 * R + 0], d1 = ld[4 * R + 1], d2 = ld[4 * R + 2], d3 = ld[4 * R + 3];                 \
        ld[4 * R + 0] = f2sub(d0, d2); ld[4 * R + 1] = f2add(d1, d2); ld[4 * R + 2] = f2sub(d2, d1); ld[4 * R + 3] = f2sub(d1, d3); \
    }
    // column pass + stash of V[i][J] for i = 0..3 into the buffer at byte address SB
#define WG_COLSTASH(J, SB)                                                                                            \
    {                                                                                                                 \
        *reinterpret_cast<float2 *>(smem_raw + (SB) + (0 * 4 + J) * 4 * PLANE) = f2sub(ld[0 + J], ld[8 + J]);            \
        *reinterpret_cast<float2 *>(smem_raw + (SB) + (1 * 4 + J) * 4 * PLANE) = f2add(ld[4 + J], ld[8 + J]);            \
        *reinterpret_cast<float2 *>(smem_raw + (SB) + (2 * 4 + J) * 4 * PLANE) = f2sub(ld[8 + J], ld[4 + J]);            \
        *reinterpret_cast<float2 *>(smem_raw + (SB) + (3 * 4 + J) * 4 * PLANE) = f2sub(ld[4 + J], ld[12 + J]);           \
    }
#define WG_BLOAD(SLOT, G) { const uintx4 v_ = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_lane, (unsigned)min((G), gmax) * BSTEP, 0); \
        breg[SLOT] = make_float4(__uint_as_float(v_.x), __uint_as_float(v_.y), __uint_as_float(v_.z), __uint_as_float(v_.w)); }

    // ---- prologue: slab 0 into buffer 0, first ring of B fragments
    {
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xbase) + (size_t)s_begin * 64, 0, xbytes - (unsigned)s_begin * 64u, 0x00020000);
#pragma unroll
        for (int i = 0; i < 16; ++i) WG_LOAD(i, xr)
#pragma unroll
        for (int u = 0; u < WG_RING; ++u) WG_BLOAD(u, s_begin * WG_STEPS + NS * xh_u + u)
        WG_ROWPASS(0) WG_ROWPASS(1) WG_ROWPASS(2) WG_ROWPASS(3)
        WG_COLSTASH(0, st_base) WG_COLSTASH(1, st_base) WG_COLSTASH(2, st_base) WG_COLSTASH(3, st_base)
    }
    __syncthreads();
    float4 afr = *reinterpret_cast<const float4 *>(smem_raw + fr_base0);    // fragment of this wave's step 0

    for (int s = s_begin; s < s_end; ++s) {
        const int sn = min(s + 1, s_end - 1);                              // next slab (last slab: harmless re-stage of itself)
        const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xbase) + (size_t)sn * 64, 0, xbytes - (unsigned)sn * 64u, 0x00020000);
        const unsigned cur = ((s - s_begin) & 1) ? WG_BUF : 0u, nxt = WG_BUF - cur;
        const unsigned sb = nxt + st_base;
        const int g0 = s * WG_STEPS + NS * xh_u;
#pragma unroll
        for (int u = 0; u < NS; ++u) {
            // (1) global loads of the next slab's patch, spread over the first half of the steps
            if (NS == 16 && u < 8) { WG_LOAD(2 * u, xr) WG_LOAD(2 * u + 1, xr) }
            if (NS == 8 && u < 4) { WG_LOAD(4 * u, xr) WG_LOAD(4 * u + 1, xr) WG_LOAD(4 * u + 2, xr) WG_LOAD(4 * u + 3, xr) }
            // (2) A fragment of the next step (step 0 of the next slab comes from the other buffer, after the barrier)
            float4 afn;
            if (u < NS - 1) afn = *reinterpret_cast<const float4 *>(smem_raw + cur + (((u + 1) & 1) ? fr_base1 : fr_base0) + (unsigned)(u + 1) * 2u * PLANE);
            else afn = *reinterpret_cast<const float4 *>(smem_raw + nxt + fr_base0);
            // (3) input transform of the next slab and its stash into the other buffer
            if (NS == 16) {
                if (u == 8) WG_ROWPASS(0)
                if (u == 9) WG_ROWPASS(1)
                if (u == 10) WG_ROWPASS(2)
                if (u == 11) { WG_ROWPASS(3) WG_COLSTASH(0, sb) }
                if (u == 12) WG_COLSTASH(1, sb)
                if (u == 13) WG_COLSTASH(2, sb)
                if (u == 14) WG_COLSTASH(3, sb)
            } else {
                if (u == 4) { WG_ROWPASS(0) WG_ROWPASS(1) }
                if (u == 5) { WG_ROWPASS(2) WG_ROWPASS(3) WG_COLSTASH(0, sb) }
                if (u == 6) { WG_COLSTASH(1, sb) WG_COLSTASH(2, sb) WG_COLSTASH(3, sb) }
            }
            // (4) the four MFMAs of step (xi = NA xh + u/2, h = u%2): channels 4(2h + half) .. +3 of the slab
            const float4 bf = breg[u % WG_RING];
            acc[u >> 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(afr.x, bf.x, acc[u >> 1], 0, 0, 0);
            acc[u >> 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(afr.y, bf.y, acc[u >> 1], 0, 0, 0);
            acc[u >> 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(afr.z, bf.z, acc[u >> 1], 0, 0, 0);
            acc[u >> 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(afr.w, bf.w, acc[u >> 1], 0, 0, 0);
            // (5) refill the ring slot just consumed: this wave's step WG_RING ahead (wraps into the next slab)
            WG_BLOAD(u % WG_RING, (u + WG_RING < NS ? g0 : g0 + WG_STEPS - NS) + u + WG_RING)
            if (u == NS - 2) __syncthreads();   // every read of `cur` is issued, every stash into `nxt` is visible
            afr = afn;
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef WG_LOAD
#undef WG_PO
#undef WG_ROWPASS
#undef WG_COLSTASH
#undef WG_BLOAD

    // ---- output transform Y = A^T M A, A^T = [[1,1,1,0],[0,1,-1,-1]]. acc[4 il + j] = M[2 xh + il][j]. Wave xh = 0 needs M_2j,
    // wave xh = 1 needs M_1j: one float4 per accumulator element through LDS ([pair][direction][r][lane] 16-byte units).
    __syncthreads();
    const bool has_res = sg.res != nullptr;
    const long pbase = p0 + wm * 32 + 4 * lhalf;
    const long pb = pbase < sg.M ? pbase : sg.M - 1;
    const int n_b = (int)(pb / HoWo);
    const int rem_b = (int)(pb - (long)n_b * HoWo);
    const int h_b = rem_b / sg.Wo, w_b = rem_b - h_b * sg.Wo;
    const bool fast = sg.Wo >= 32;
    const int co = n0 + wn * 32 + l32;
    const bool co_ok = co < p.Cout;
    const float bv = (p.bias != nullptr && co_ok) ? p.bias[co] : 0.f;
    // position of accumulator element with row offset `off` inside the block; false if it is beyond the map
#define WG_WHERE(OFF, N_, H_, W_)                                                                                     \
    int N_ = n_b, H_ = h_b, W_ = w_b;                                                                                 \
    if (fast) {                                                                                                       \
        W_ += (OFF);                                                                                                  \
        if (W_ >= sg.Wo) { W_ -= sg.Wo; ++H_; }                                                                       \
        if (H_ >= sg.Ho) { H_ -= sg.Ho; ++N_; }                                                                       \
    } else {                                                                                                          \
        const long pp_ = pbase + (OFF);                                                                               \
        N_ = (int)(pp_ / HoWo);                                                                                       \
        const int rem_ = (int)(pp_ - (long)N_ * HoWo);                                                                \
        H_ = rem_ / sg.Wo; W_ = rem_ - H_ * sg.Wo;                                                                    \
    }
    // one output row (two pixels) of a tile: + bias, + residual, ReLU, store (split-K: raw partial sums). r08: 32-bit byte offsets
    // through buffer descriptors (r07 built a 64-bit element index per row: ~15 VALU instructions for each of the 16-32 rows of a
    // lane); the second pixel of a row that falls beyond the map is an out-of-range offset (load 0 / store dropped).
    const unsigned crow = (unsigned)p.Cout * 4u;
    const unsigned co4 = 4u * (unsigned)co;
    const size_t oaddr_ = reinterpret_cast<size_t>(SPLITK ? (float *)(p.partial + (long)kz * p.m_total * p.Cout) : sg.out);
    const unsigned obytes_ = __builtin_amdgcn_readfirstlane((unsigned)(SPLITK ? p.m_total : (long)sg.N * sg.OH * sg.OW) * crow);
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(oaddr_ >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)oaddr_)),
        0, (int)obytes_, 0x00020000);
    const size_t raddr_ = reinterpret_cast<size_t>(has_res ? sg.res : sg.out);
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(
        reinterpret_cast<void *>(((size_t)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(raddr_ >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((unsigned)raddr_)),
        0, (int)__builtin_amdgcn_readfirstlane((unsigned)((long)sg.N * sg.OH * sg.OW) * crow), 0x00020000);
#define WG_STORE_ROW(N_, OY, OX, V0, V1)                                                                              \
    if ((OY) < sg.OH) {                                                                                               \
        float v0_ = (V0), v1_ = (V1);                                                                                 \
        const unsigned o0_ = (unsigned)(((N_) * sg.OH + (OY)) * sg.OW + (OX)) * crow + co4;                           \
        const unsigned o1_ = ((OX) + 1 < sg.OW) ? o0_ + crow : 0x80000000u;                                           \
        if (!SPLITK) {                                                                                                \
            v0_ = v0_ + bv; v1_ = v1_ + bv;                                                                           \
            if (has_res) {                                                                                            \
                v0_ = v0_ + __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, o0_, 0, 0));                  \
                v1_ = v1_ + __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, o1_, 0, 0));                  \
            }                                                                                                         \
            if (p.relu) { v0_ = fmaxf(v0_, 0.f); v1_ = fmaxf(v1_, 0.f); }                                             \
        }                                                                                                             \
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v0_), orsrc, o0_, 0, 0);                                \
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v1_), orsrc, o1_, 0, 0);                                \
    }
    if constexpr (NX == 2) {
        float4 *mine = reinterpret_cast<float4 *>(smem_raw + pair * 32768 + xh_u * 16384) + lane;
        const float4 *theirs = reinterpret_cast<const float4 *>(smem_raw + pair * 32768 + (1 - xh_u) * 16384) + lane;
        if (xh_u == 0) {                    // xh = 0 gives M_1j = acc[4 + j], xh = 1 gives M_2j = acc[j]
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[r * 64] = make_float4(acc[4][r], acc[5][r], acc[6][r], acc[7][r]);
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) mine[r * 64] = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int off = (r & 3) + 8 * (r >> 2);
            const float4 o = theirs[r * 64];
            if (!(co_ok && pbase + off < sg.M)) continue;
            WG_WHERE(off, n, h, w)
            // t[j] = sum_i A^T[xh][i] M[i][j]: row 0: (M0j + M1j) + M2j, row 1: (M1j - M2j) - M3j
            float t0, t1, t2, t3;
            if (xh_u == 0) {
                t0 = (acc[0][r] + acc[4][r]) + o.x; t1 = (acc[1][r] + acc[5][r]) + o.y;
                t2 = (acc[2][r] + acc[6][r]) + o.z; t3 = (acc[3][r] + acc[7][r]) + o.w;
            } else {
                t0 = (o.x - acc[0][r]) - acc[4][r]; t1 = (o.y - acc[1][r]) - acc[5][r];
                t2 = (o.z - acc[2][r]) - acc[6][r]; t3 = (o.w - acc[3][r]) - acc[7][r];
            }
            WG_STORE_ROW(n, 2 * h + xh_u, 2 * w, (t0 + t1) + t2, (t1 - t2) - t3)
        }
    } else {
        // four waves per block: wave xh holds M[xh][0..3] (acc[j]); every wave publishes its row, then finishes the accumulator
        // elements r in [4 xh, 4 xh + 4) -- both output rows of those tiles -- from the four published rows
        float4 *mine = reinterpret_cast<float4 *>(smem_raw + xh_u * 16384) + lane;
#pragma unroll
        for (int r = 0; r < 16; ++r) mine[r * 64] = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int r = 4 * xh_u + rr;
            const int off = rr + 8 * xh_u;      // (r & 3) + 8 (r >> 2)
            const float4 m0 = reinterpret_cast<const float4 *>(smem_raw)[r * 64 + lane];
            const float4 m1 = reinterpret_cast<const float4 *>(smem_raw + 16384)[r * 64 + lane];
            const float4 m2 = reinterpret_cast<const float4 *>(smem_raw + 32768)[r * 64 + lane];
            const float4 m3 = reinterpret_cast<const float4 *>(smem_raw + 49152)[r * 64 + lane];
            if (!(co_ok && pbase + off < sg.M)) continue;
            WG_WHERE(off, n, h, w)
            const float a0 = (m0.x + m1.x) + m2.x, a1 = (m0.y + m1.y) + m2.y, a2 = (m0.z + m1.z) + m2.z, a3 = (m0.w + m1.w) + m2.w;
            const float b0 = (m1.x - m2.x) - m3.x, b1 = (m1.y - m2.y) - m3.y, b2 = (m1.z - m2.z) - m3.z, b3 = (m1.w - m2.w) - m3.w;
            WG_STORE_ROW(n, 2 * h, 2 * w, (a0 + a1) + a2, (a1 - a2) - a3)
            WG_STORE_ROW(n, 2 * h + 1, 2 * w, (b0 + b1) + b2, (b1 - b2) - b3)
        }
    }
#undef WG_WHERE
#undef WG_STORE_ROW
}

template <bool SPLITK, int TM, int TN>
__global__ void __launch_bounds__(8 * TM, TM == 64 ? 1 : 2) conv_wino16_f32_kernel(const ConvParams p)
{
    conv_wino16_body<SPLITK, TM, TN>(p, (int)blockIdx.x);
}

// r10: a launch whose 32 x 64 tiling ends in a nearly empty last round (the mask head: 100 ROIs = 616 workgroups for 512 slots) as ONE
// launch of two forms: workgroups [0, main_grid) are the 32 x 64 tiles of the first images (pm: as many as fill whole rounds), the rest
// 32 x 32 tiles of the remaining images (pt, weights in the 32-channel packing) -- half the work each, dealt out by the dispatcher as the
// main workgroups retire, so the tail of the launch is balanced over the CUs instead of leaving most of them idle behind a few full-size
// stragglers. Same arithmetic per output element as either form alone (bit-identical).
__global__ void __launch_bounds__(256, 2) conv_wino16_tail_f32_kernel(const ConvParams pm, const ConvParams pt, const int main_grid)
{
    if ((int)blockIdx.x < main_grid) conv_wino16_body<false, 32, 64>(pm, (int)blockIdx.x);
    else conv_wino16_body<false, 32, 32>(pt, (int)blockIdx.x - main_grid);
}

// Launch: p is a filled 3x3 / stride 1 / pad 1 description (conv_fill) whose Ho, Wo already count 2x2 output tiles.
// p.ksplit > 1: one map, partial sums into p.partial (the caller runs the reduction).
template <int TM, int TN>
static int conv_wino16_launch_tm(hipStream_t st, ConvParams &p)
{
    int tiles = 0;
    for (int i = 0; i < p.nseg; ++i) { p.seg[i].tile_start = tiles; tiles += (int)((p.seg[i].M + TM - 1) / TM); }
    p.m_tiles = tiles;
    p.n_tiles = p.ldw / TN;
    // (no static LDS. The 64-tile form owns a CU by construction; the 32-tile forms, two per CU, take a residency cap: residency.h)
    const size_t own = 2 * 16 * 4 * TM * 16;
    const size_t smem = TM == 32 ? res_dynamic_lds(TN == 64 ? RES_WINO16_32X64 : RES_WINO16_32X32, 0, own) : own;
    const int smem_max = TM == 32 ? res_max_dynamic(0) : (int)own;
    static std::atomic<unsigned long long> attr_dev{0};
    UPS_ONCE_PER_DEVICE(attr_dev,
        UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_wino16_f32_kernel<false, TM, TN>), hipFuncAttributeMaxDynamicSharedMemorySize, smem_max));
        UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_wino16_f32_kernel<true, TM, TN>), hipFuncAttributeMaxDynamicSharedMemorySize, smem_max)));
    const int grid = 8 * ((p.m_tiles + 7) / 8) * p.n_tiles;
    if (p.ksplit > 1) hipLaunchKernelGGL((conv_wino16_f32_kernel<true, TM, TN>), dim3(grid * p.ksplit), dim3(8 * TM), smem, st, p);
    else hipLaunchKernelGGL((conv_wino16_f32_kernel<false, TM, TN>), dim3(grid), dim3(8 * TM), smem, st, p);
    UPS_CHECK_LAUNCH("conv_wino16_f32_kernel");
    ups_set_form("wino<%d,%d,%d>", p.ksplit > 1 ? 1 : 0, TM, TN);
    return 0;
}

// Launch: p is a filled 3x3 / stride 1 / pad 1 description (conv_fill) whose Ho, Wo already count 2x2 output tiles.
// p.ksplit > 1: one map, partial sums into p.partial (the caller runs the reduction). The channel tile follows the packing:
// ldw == 32 (Cout <= 32, packed in 32-channel fragment order) -> the 32x32 form; otherwise ldw % 64 == 0.
int g_wino_tm = 0;   // 0 auto; 32 / 64 forced (upsnet_conv_tuning, A/B runs)
static int conv_wino16_launch(hipStream_t st, ConvParams &p, int tn32 = 0)
{
    UPS_REQUIRE(p.Cin % 16 == 0 && (p.ldw == 32 || p.ldw % 64 == 0 || (tn32 && p.ldw % 32 == 0)), "conv2d_winograd_nhwc_f32: Cin %% 16 must be 0 and ldw 32 or a multiple of 64");
    for (int i = 0; i < p.nseg; ++i) {
        UPS_REQUIRE((long)p.seg[i].N * p.seg[i].H * p.seg[i].W * p.Cin < (1L << 28), "conv2d_winograd_nhwc_f32: feature map %d exceeds 1 GiB; split the batch", i);
        UPS_REQUIRE((long)p.seg[i].N * p.seg[i].OH * p.seg[i].OW * p.Cout < (1L << 29), "conv2d_winograd_nhwc_f32: output %d exceeds 2 GiB; split the batch", i);
    }
    if (p.ksplit > 1) {
        const int nslabs = p.Cin / 16;
        UPS_REQUIRE(p.nseg == 1 && p.partial, "conv2d_winograd_nhwc_f32_splitk: one map and a workspace");
        UPS_REQUIRE(((nslabs + p.ksplit - 1) / p.ksplit) * (p.ksplit - 1) < nslabs, "conv2d_winograd_nhwc_f32_splitk: %d K slabs cannot be split %d ways", nslabs, p.ksplit);
        p.m_total = (long)p.seg[0].N * p.seg[0].OH * p.seg[0].OW;
    }
    if (p.ldw == 32 || tn32) {   // 32-channel workgroups: narrow heads, or on request (weights packed with tn = 32): every ldw % 32 == 0
        UPS_REQUIRE(p.ldw % 32 == 0, "conv2d_winograd_nhwc_f32: the 32-channel form needs ldw %% 32 == 0");
        return conv_wino16_launch_tm<32, 32>(st, p);
    }
    // 64-tile workgroups (one per CU) for the big maps, where the doubled B traffic of the 32-tile form costs more than its
    // overlapped prologue / epilogue gains (FPN P2: 638 vs 733 us); 32-tile workgroups (two per CU) below 768 of the former
    // (FPN P4 78 -> 49 us, res4 conv2 73 -> 46, mask head 148 -> 116; equal at P3 / the RPN launch). hipconv._wino_tm mirrors this.
    long wgs64 = 0;
    for (int i = 0; i < p.nseg; ++i) wgs64 += (p.seg[i].M + 63) / 64;
    wgs64 *= p.ldw / 64;
    static const long tm64_min = getenv("UPSNET_WINO_TM64_MIN") ? atol(getenv("UPSNET_WINO_TM64_MIN")) : 768;   // (models/hipconv.py reads the same)
    const int tm = g_wino_tm ? g_wino_tm : (wgs64 > tm64_min ? 64 : 32);
    return tm == 32 ? conv_wino16_launch_tm<32, 64>(st, p) : conv_wino16_launch_tm<64, 64>(st, p);
}

// weight [Cout, Cin, 3, 3] -> U = G g G^T, G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]], stored in fragment order
// [n-tile = co/TN][slab = c/16][xi = 4i+j][q = (c%16)/4][co%TN][c%4] (16 * Cin * ldw floats; TN = 64 and ldw = Cout rounded up to
// 64, or TN = ldw = 32 for Cout <= 32)
__global__ void conv_pack_weight_wino16_kernel(const float *__restrict__ w, int cout, int cin, int ldw, int tn, float *__restrict__ wp)
{
    const long total = (long)ldw * cin;
    const int nslabs = cin >> 4;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)blockDim.x * gridDim.x) {
        const int co = idx % ldw, c = idx / ldw;
        float g[3][3], t[4][3], u[4][4];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) g[a][b] = co < cout ? w[(((long)co * cin + c) * 3 + a) * 3 + b] : 0.f;
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            t[0][b] = g[0][b];
            t[1][b] = 0.5f * ((g[0][b] + g[1][b]) + g[2][b]);
            t[2][b] = 0.5f * ((g[0][b] - g[1][b]) + g[2][b]);
            t[3][b] = g[2][b];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            u[a][0] = t[a][0];
            u[a][1] = 0.5f * ((t[a][0] + t[a][1]) + t[a][2]);
            u[a][2] = 0.5f * ((t[a][0] - t[a][1]) + t[a][2]);
            u[a][3] = t[a][2];
        }
        const long blk = ((long)(co / tn) * nslabs + (c >> 4)) * 16;
        const int q = (c & 15) >> 2, ci = c & 3, cl = co % tn;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) wp[(((blk + a * 4 + b) * 4 + q) * tn + cl) * 4 + ci] = u[a][b];
    }
}

static int wino_pack(void *stream, const float *weight, int cout, int cin, int ldw, int tn, float *wpack)
{
    UPS_REQUIRE(weight && wpack && cout > 0 && cin > 0 && ldw >= cout, "conv_pack_weight_winograd: bad args");
    UPS_REQUIRE(cin % 16 == 0 && (tn == 32 || tn == 64) && ldw % tn == 0, "conv_pack_weight_winograd: Cin %% 16 must be 0 and ldw a multiple of the channel tile");
    const long total = (long)ldw * cin;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 65535) blocks = 65535;
    hipLaunchKernelGGL(conv_pack_weight_wino16_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, cout, cin, ldw, tn, wpack);
    UPS_CHECK_LAUNCH("conv_pack_weight_wino16_kernel");
    return 0;
}

extern "C" int upsnet_conv_pack_weight_winograd(void *stream, const float *weight, int cout, int cin, int ldw, float *wpack)
{
    UPS_REQUIRE(ldw == 32 || ldw % 64 == 0, "conv_pack_weight_winograd: ldw 32 or a multiple of 64");
    return wino_pack(stream, weight, cout, cin, ldw, ldw == 32 ? 32 : 64, wpack);
}

/* The same U = G g G^T in the fragment order of the 32-CHANNEL workgroup form for any Cout (ldw = Cout rounded up to 32): the operand
 * of upsnet_conv2d_winograd_nhwc_f32_tn32. */
extern "C" int upsnet_conv_pack_weight_winograd_tn32(void *stream, const float *weight, int cout, int cin, int ldw, float *wpack)
{
    return wino_pack(stream, weight, cout, cin, ldw, 32, wpack);
}

// geometry of the 3x3 / stride 1 / pad 1 convolution first (conv_fill), then the GEMM rows become 2x2 output tiles
static int wino_fill(ConvParams &p, const char *who, int nseg, const float *const x[], const float *const residual[], float *const out[],
                     const int batch[], const int height[], const int width[], int Cin, int Cout, const float *wpack, int ldw,
                     const float *bias, int relu)
{
    int rc = conv_fill(p, who, nseg, x, residual, nullptr, nullptr, out, batch, height, width, Cin, Cout, wpack, ldw, bias, 3, 3, 1, 1, 1, relu);
    if (rc) return rc;
    UPS_REQUIRE((long)16 * Cin * ldw < (1L << 30), "%s: packed weight exceeds 4 GiB", who);
    for (int i = 0; i < nseg; ++i) {
        ConvSeg &s = p.seg[i];
        s.OH = s.Ho; s.OW = s.Wo;
        s.Ho = (s.OH + 1) / 2; s.Wo = (s.OW + 1) / 2;
        s.M = (long)s.N * s.Ho * s.Wo;
    }
    return 0;
}

extern "C" int upsnet_conv2d_winograd_nhwc_f32(void *stream, int nseg, const float *const x[], const float *const residual[],
                                               float *const out[], const int batch[], const int height[], const int width[], int Cin,
                                               const float *wpack, int ldw, const float *bias, int Cout, int relu)
{
    ConvParams p;
    int rc = wino_fill(p, "conv2d_winograd_nhwc_f32", nseg, x, residual, out, batch, height, width, Cin, Cout, wpack, ldw, bias, relu);
    if (rc) return rc;
    return conv_wino16_launch((hipStream_t)stream, p);
}

/* upsnet_conv2d_winograd_nhwc_f32 on 32-tile x 32-CHANNEL workgroups whatever Cout (wpack from upsnet_conv_pack_weight_winograd_tn32,
 * ldw % 32 == 0): twice the workgroups of the 32 x 64 form with half the work each -- for launches whose 32 x 64 tiling ends in a
 * nearly empty last round (the tail ROIs of the mask head, models/hipconv.py). Same arithmetic in the same order as the other forms:
 * bit-identical results. */
extern "C" int upsnet_conv2d_winograd_nhwc_f32_tn32(void *stream, int nseg, const float *const x[], const float *const residual[],
                                                    float *const out[], const int batch[], const int height[], const int width[], int Cin,
                                                    const float *wpack, int ldw, const float *bias, int Cout, int relu)
{
    ConvParams p;
    int rc = wino_fill(p, "conv2d_winograd_nhwc_f32_tn32", nseg, x, residual, out, batch, height, width, Cin, Cout, wpack, ldw, bias, relu);
    if (rc) return rc;
    return conv_wino16_launch((hipStream_t)stream, p, 1);
}

/* One launch over a batch x [N, H, W, Cin]: images [0, n_main) on 32-tile x 64-channel workgroups (wpack / ldw from
 * upsnet_conv_pack_weight_winograd), images [n_main, N) on 32 x 32 workgroups (wpack32 / ldw32 from ..._winograd_tn32) -- see
 * conv_wino16_tail_f32_kernel. out [N, H, W, Cout]. Bit-identical to upsnet_conv2d_winograd_nhwc_f32 on the whole batch. */
extern "C" int upsnet_conv2d_winograd_nhwc_f32_tail(void *stream, const float *x, float *out, int batch, int n_main, int height, int width,
                                                    int Cin, const float *wpack, int ldw, const float *wpack32, int ldw32, const float *bias,
                                                    int Cout, int relu)
{
    UPS_REQUIRE(x && out && wpack && wpack32 && n_main > 0 && n_main < batch && ldw % 64 == 0 && ldw32 % 32 == 0 && Cin % 16 == 0,
                "conv2d_winograd_nhwc_f32_tail: 0 < n_main < batch, ldw %% 64 == 0, ldw32 %% 32 == 0, Cin %% 16 == 0");
    ConvParams pm, pt;
    const float *xm[1] = {x}, *xt[1] = {x + (size_t)n_main * height * width * Cin};
    float *om[1] = {out}, *ot[1] = {out + (size_t)n_main * height * width * Cout};
    const int nm[1] = {n_main}, nt[1] = {batch - n_main}, hh[1] = {height}, ww[1] = {width};
    int rc = wino_fill(pm, "conv2d_winograd_nhwc_f32_tail", 1, xm, nullptr, om, nm, hh, ww, Cin, Cout, wpack, ldw, bias, relu);
    if (rc) return rc;
    rc = wino_fill(pt, "conv2d_winograd_nhwc_f32_tail", 1, xt, nullptr, ot, nt, hh, ww, Cin, Cout, wpack32, ldw32, bias, relu);
    if (rc) return rc;
    UPS_REQUIRE((long)batch * height * width * Cin < (1L << 28) && (long)batch * height * width * Cout < (1L << 29),
                "conv2d_winograd_nhwc_f32_tail: feature map exceeds 1 GiB; split the batch");
    pm.seg[0].tile_start = 0; pm.m_tiles = (int)((pm.seg[0].M + 31) / 32); pm.n_tiles = ldw / 64;
    pt.seg[0].tile_start = 0; pt.m_tiles = (int)((pt.seg[0].M + 31) / 32); pt.n_tiles = ldw32 / 32;
    const int main_grid = 8 * ((pm.m_tiles + 7) / 8) * pm.n_tiles, tail_grid = 8 * ((pt.m_tiles + 7) / 8) * pt.n_tiles;
    const size_t smem = 2 * 16 * 4 * 32 * 16;
    static std::atomic<unsigned long long> attr_dev{0};
    UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conv_wino16_tail_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)));
    hipLaunchKernelGGL(conv_wino16_tail_f32_kernel, dim3(main_grid + tail_grid), dim3(256), smem, (hipStream_t)stream, pm, pt, main_grid);
    UPS_CHECK_LAUNCH("conv_wino16_tail_f32_kernel");
    ups_set_form("wino_tail<%d,%d>", main_grid, tail_grid);
    return 0;
}

extern "C" int upsnet_conv2d_winograd_nhwc_f32_splitk(void *stream, const float *x, const float *residual, float *out, int batch, int height,
                                                      int width, int Cin, const float *wpack, int ldw, const float *bias, int Cout, int relu,
                                                      int ksplit, void *workspace)
{
    const float *xs[1] = {x};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    int rc = wino_fill(p, "conv2d_winograd_nhwc_f32_splitk", 1, xs, nullptr, os, nb, hh, ww, Cin, Cout, wpack, ldw, bias, relu);
    if (rc) return rc;
    UPS_REQUIRE(workspace && ksplit >= 2 && ksplit <= 8, "conv2d_winograd_nhwc_f32_splitk: ksplit must be 2..8 and a workspace given");
    UPS_REQUIRE(Cout % 4 == 0, "conv2d_winograd_nhwc_f32_splitk: Cout must be a multiple of 4");
    p.ksplit = ksplit;
    p.partial = (float *)workspace;
    rc = conv_wino16_launch((hipStream_t)stream, p);
    if (rc) return rc;
    return conv_splitk_reduce((hipStream_t)stream, p.partial, ksplit, p.m_total, p.m_total, Cout, bias, residual, relu, out);
}
