// conv1x1.hip -- 1x1 convolution (stride 1 / 2) as a lean fp32 MFMA GEMM: out[pixel, co] = sum_c x[pixel, c] * w[co, c].
//
// Reference: the 1x1 nn.Conv2d layers of the ResNet bottlenecks (conv1 / conv3 / downsample, upsnet/models/resnet.py:53-100)
// and the FPN laterals with their top-down add (fpn.py:78-104), each followed by separate frozen-BN / ReLU / add passes.
//
// Why a second kernel next to conv_igemm_f32_kernel (conv.hip): per image the 1x1 layers are 36 of the 48 direct launches and
// ran at 52-65 % of the attainable fp32 MFMA rate (profiles/r05, r06g). The general kernel pays for its generality exactly
// there: one ds_read_b32 per operand and MFMA (2 LDS reads per MFMA), four ds_write_b32 per staged float4 (the [k][pixel]
// transposition), B through LDS, ~100 address instructions per tap change. A 1x1 convolution on NHWC needs none of it:
//   * A: a lane's MFMA fragment is four CONSECUTIVE channels of one pixel = the float4 the loader already holds. It is staged
//     with one ds_write_b128 into 16-byte units [channel quarter][pixel ^ swizzle] and read back with one ds_read_b128 per four
//     (BN = 64) or eight (BN = 128) MFMAs -- conflict-free both ways (same layout as deform_fused.hip / conv_wino.hip).
//   * B never touches LDS: packed in fragment order (upsnet_dcn_pack_weight with kh = kw = 1) it is one 16-byte buffer load per
//     lane and step from L2, prefetched four steps ahead in a register ring.
//   * a K step (32 channels) costs a thread 2 global loads + 2 LDS writes; the loads of step s+2 are issued while step s is
//     contracted (8 registers), pixels beyond the map read as 0 through the buffer bounds check.
// Tile: 64 pixels x 128 channels (4 waves = 4 column blocks x both row blocks) or 64 x 64 (2 x 2 waves) for Cout <= 64 and for
// maps with few tiles. (Measured and rejected: different s_setprio levels for the four workgroups of a CU, to stagger their
// completion so that the stores of one overlap the K walk of the others: 0-4 %, within noise.) Epilogue fused: + bias (folded frozen-BN shift), + residual (optionally read through the FPN's nearest x2
// upsampling), ReLU, one NHWC store. Fixed accumulation order (bit-repeatable).
#include "conv_params.h"
#include "residency.h"
#include "upsnet_hip.h"

typedef unsigned uintx4 __attribute__((ext_vector_type(4)));

#define C1_BM 64

// NW: waves along N (4: BN = 128, every wave owns both 32-row blocks of one column block; 2: BN = 64, waves 2 x 2).
// MODE 1 (RESUP): the residual lives at half resolution and is read through a nearest x2 upsampling (fpn.py:34,90-96).
// MODE 2: 2x2 / stride-2 transposed convolution (the mask head's upsampling layer, rcnn.py:132-133) as the GEMM [N H W, Cin] x [Cin, 4 C]
// with columns (dy, dx, c): the epilogue scatters row (n, h, w) / column (dy, dx, c) to output pixel (2h + dy, 2w + dx), channel c. A
// 32-column block lies inside one (dy, dx) (C % 32 == 0), so (dy, dx) is wave-uniform; the per-row part of the output offset is
// tabulated once per workgroup in LDS (one division chain per row instead of one per accumulator element).
// A K step (32 channels, one barrier) is 4 sub-steps of 8 channels (one A fragment, one B fragment, 4 NR MFMAs each). The
// activations of step t+2 are fetched in sub-step 2 of step t and stashed in sub-step 1 of step t+1. Every load in the loop is
// unconditional (steps beyond the end read through an out-of-range offset = 0, no memory access) and the prologue issues its loads
// in the order of a steady-state step, so the vmcnt values the compiler derives for the loop are exact: with a conditional fetch
// it fell back to vmcnt(3) everywhere, which -- vmcnt retires in order -- made every B wait also a wait for the activations
// fetched two sub-steps earlier (5-15 % per layer). (Measured and rejected: two slabs per step with a B ring of 8, i.e. 7
// sub-steps of latency cover and half the barriers: 2-10 % slower on every layer -- latency is not what bounds the loop.)
template <int NW, int MODE>
__global__ void __launch_bounds__(256, 4) conv1x1_frag_f32_kernel(const ConvParams p)
{
    constexpr bool RESUP = MODE == 1;
    constexpr bool SPLITK = MODE == 3;
    constexpr int NR = NW == 4 ? 2 : 1;          // 32-row blocks per wave
    constexpr int NU = 4;                        // sub-steps per step = B fragments in flight
    constexpr int C1_ABUF = 8 * C1_BM;           // float4 units of one A buffer: 8 channel quarters x 64 pixels
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float4 *As = reinterpret_cast<float4 *>(smem_raw);   // [2][8 q][64 px ^ 2q]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lhalf = lane >> 5, l32 = lane & 31;
    const int wn = NW == 4 ? wave : (wave >> 1), wm = NW == 4 ? 0 : (wave & 1);
    // XCD-aware tile order (workgroup b runs on XCD b % 8): contiguous m-tile range per XCD, all n-tiles of an m-tile together
    int m_t, n_t, kz = 0;
    {
        const int nt = p.n_tiles;
        const int per = (p.m_tiles + 7) >> 3;
        int bid = (int)blockIdx.x;
        if (SPLITK) { const int base_grid = 8 * per * nt; kz = bid / base_grid; bid -= kz * base_grid; }
        const int qq = bid >> 3;
        n_t = qq % nt;
        const int local = qq / nt;
        m_t = (bid & 7) * per + local;
        if (local >= per || m_t >= p.m_tiles) return;
    }
    const ConvSeg sg = p.seg[0];
    const long p0 = (long)m_t * C1_BM;
    const int nsl = p.Cin >> 5;                  // K steps (32-channel slabs)
    // MODE 3 (split-K): workgroup (tile, kz) walks steps [s_begin, s_end) and leaves raw partial sums in p.partial (launcher: never empty)
    const int s_per = SPLITK ? (nsl + p.ksplit - 1) / p.ksplit : nsl;
    const int s_begin = SPLITK ? kz * s_per : 0, s_end = SPLITK ? min(s_begin + s_per, nsl) : nsl;
    const long HoWo = (long)sg.Ho * sg.Wo;

    // ---- loader geometry: thread = (pixel prow [+32], channel quarter q); byte offset of the pixel's channel vector, bit 31 set
    // beyond the map (the buffer load then returns 0)
    const int q = tid & 7, prow = tid >> 3;
    unsigned po0, po1;
    {
        unsigned po[2];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const long pp = p0 + prow + 32 * r;
            po[r] = 0x80000000u;
            if (pp < sg.M) {
                const int n = (int)(pp / HoWo);
                const int rem = (int)(pp - (long)n * HoWo);
                const int ho = rem / sg.Wo, wo = rem - ho * sg.Wo;
                po[r] = (unsigned)((n * sg.H + ho * p.stride) * sg.W + wo * p.stride) * 4u * (unsigned)p.Cin + 16u * (unsigned)q;
            }
        }
        po0 = po[0]; po1 = po[1];
    }
    const size_t xaddr = reinterpret_cast<size_t>(sg.x);
    const unsigned xlo = __builtin_amdgcn_readfirstlane((unsigned)xaddr), xhi = __builtin_amdgcn_readfirstlane((unsigned)(xaddr >> 32));
    const unsigned xbytes = __builtin_amdgcn_readfirstlane((unsigned)(sg.N * sg.H * sg.W) * 4u * (unsigned)p.Cin);
    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)xhi << 32) | xlo), 0, (int)xbytes, 0x00020000);
    const unsigned st0 = (unsigned)(q * C1_BM + (prow ^ (2 * q))), st1 = (unsigned)(q * C1_BM + ((prow + 32) ^ (2 * q)));
    // B: lane's float4 of global step g = 4 s + h sits at wbase(cb) + g * 1024 + lhalf * 512 + l32 * 16
    const int cb = NW * n_t + wn;
    const size_t waddr = reinterpret_cast<size_t>(p.w) + (size_t)cb * (size_t)nsl * 4096u;
    const unsigned wlo = __builtin_amdgcn_readfirstlane((unsigned)waddr), whi = __builtin_amdgcn_readfirstlane((unsigned)(waddr >> 32));
    const __amdgpu_buffer_rsrc_t wrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)whi << 32) | wlo), 0, nsl * 4096, 0x00020000);
    const unsigned b_lane = (unsigned)(lhalf * 512 + l32 * 16);
    const int gmax = s_end * 4 - 1;

    floatx16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    float4 xa0, xa1;          // staged pixels of the K step in flight
    float4 breg[NU];

#define C1_LDX(D, O) { const uintx4 v_ = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, (O), 0, 0); \
        D = make_float4(__uint_as_float(v_.x), __uint_as_float(v_.y), __uint_as_float(v_.z), __uint_as_float(v_.w)); }
    // step S: channels 32 S ... of the two pixels; a step beyond the end reads nothing (offset out of range -> 0)
#define C1_FETCH(S, D0, D1) { const unsigned c_ = (S) < s_end ? (unsigned)(S) * 128u : 0x80000000u; C1_LDX(D0, po0 + c_) C1_LDX(D1, po1 + c_) }
#define C1_STASH(BUF, D0, D1) { As[(BUF) * C1_ABUF + st0] = D0; As[(BUF) * C1_ABUF + st1] = D1; }
#define C1_BLOAD(SLOT, G) { const uintx4 v_ = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, b_lane, (unsigned)min((G), gmax) * 1024u, 0); \
        breg[SLOT] = make_float4(__uint_as_float(v_.x), __uint_as_float(v_.y), __uint_as_float(v_.z), __uint_as_float(v_.w)); }
    // fragment of sub-step H: channel quarter 2 H + lhalf of the step
#define C1_FRAG(BUF, H, A0, A1)                                                                                        \
    {                                                                                                                  \
        const int q_ = 2 * (H) + lhalf;                                                                                \
        A0 = As[(BUF) * C1_ABUF + q_ * C1_BM + ((32 * wm + l32) ^ (2 * q_))];                                          \
        if (NR == 2) A1 = As[(BUF) * C1_ABUF + q_ * C1_BM + ((32 + l32) ^ (2 * q_))];                                  \
    }

    // ---- prologue: step 0 -> buffer 0, step 1 in flight, first ring of B fragments. The loads are issued in the order of a
    // steady-state step (B of sub-steps 0 and 1, the activations, the remaining B), so that the wait counts the compiler derives
    // for the loop -- the merge of this entry state and the back edge -- are the steady-state ones, not more conservative.
    {
        float4 xp0, xp1;
        C1_FETCH(s_begin, xp0, xp1)
        C1_BLOAD(0, 4 * s_begin)
        C1_BLOAD(1, 4 * s_begin + 1)
        C1_FETCH(s_begin + 1, xa0, xa1)
        C1_BLOAD(2, 4 * s_begin + 2)
        C1_BLOAD(3, 4 * s_begin + 3)
        C1_STASH(0, xp0, xp1)
    }
    __syncthreads();
    float4 a0, a1;
    C1_FRAG(0, 0, a0, a1)
    // The K steps are walked in PAIRS with the LDS buffer index static (step t in buffer 0, t + 1 in buffer 1): every LDS address of the loop
    // is an immediate and the loop has one form (as `cur = (t - s_begin) & 1` the compiler unrolled it by two itself and kept a remainder
    // copy, across which it spilled 5 registers). An odd number of steps ends in one step past s_end: its activations read as 0 (C1_FETCH),
    // its weights are the last valid ones (C1_BLOAD clamps), so it adds exact zeros -- for FINITE weights (an Inf / NaN weight in the last
    // slab of an odd-step layer would turn 0 x Inf into NaN; include/upsnet_hip.h states the assumption). Peeling the odd step behind the
    // loop instead was tried in r11 and not kept: it changes the register allocation of the loop (96 -> 100, the 64-wide form 70 -> 75 =
    // one wave per SIMD less) for a case no layer of the models has (Cin / 32 is even everywhere; tests cover 1, 3 and 5 steps).
#define C1_STEP(T, CUR)                                                                                                \
    _Pragma("unroll") for (int u = 0; u < NU; ++u) {                                                                   \
        float4 n0_, n1_;                                                                                               \
        if (u < NU - 1) C1_FRAG(CUR, u + 1, n0_, n1_)                                                                  \
        if (u == 1) C1_STASH((CUR) ^ 1, xa0, xa1)         /* step T+1 (fetched during step T-1); after the last step: zeros, unread */ \
        if (u == 2) C1_FETCH((T) + 2, xa0, xa1)                                                                        \
        if (u == NU - 1) { __syncthreads(); C1_FRAG((CUR) ^ 1, 0, n0_, n1_) }                                          \
        const float4 bf_ = breg[u];                                                                                    \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, bf_.x, acc0, 0, 0, 0);                                       \
        if (NR == 2) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, bf_.x, acc1, 0, 0, 0);                          \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, bf_.y, acc0, 0, 0, 0);                                       \
        if (NR == 2) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, bf_.y, acc1, 0, 0, 0);                          \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, bf_.z, acc0, 0, 0, 0);                                       \
        if (NR == 2) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, bf_.z, acc1, 0, 0, 0);                          \
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, bf_.w, acc0, 0, 0, 0);                                       \
        if (NR == 2) acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, bf_.w, acc1, 0, 0, 0);                          \
        C1_BLOAD(u, g + NU + u)                                                                                        \
        a0 = n0_;                                                                                                      \
        if (NR == 2) a1 = n1_;                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
    }                                                                                                                  \
    g += NU;
    int g = 4 * s_begin;
    for (int t = s_begin; t < s_end; t += 2) {
        C1_STEP(t, 0)
        C1_STEP(t + 1, 1)
    }
#undef C1_STEP
#undef C1_LDX
#undef C1_FETCH
#undef C1_STASH
#undef C1_BLOAD
#undef C1_FRAG

    // ---- epilogue: + bias, + residual (RESUP: through the nearest x2 upsampling), ReLU, NHWC store. Accumulator element r of
    // lane (lhalf, l32): row 8 (r >> 2) + 4 lhalf + (r & 3), column l32 of the 32x32 block.
    // r08: residual loads and stores go through buffer descriptors: one loop-invariant lane offset (its column + its row half) and a
    // SCALAR row offset per element -- no 64-bit address arithmetic per element (r07: ~8 VALU instructions for each of the 64 loads /
    // stores of a lane, and 5 spilled registers in the 128-wide form); rows beyond the map and padded columns are out-of-range
    // offsets (loads return 0, stores are dropped), so there is no per-element predicate either.
    // Sibling launch (MODE 0, p.sib_split > 0: conv1 and the projection shortcut of a stage's first bottleneck read the same input): this
    // wave's 32-column block belongs to the first layer (columns below the split: its own output tensor, width, ReLU flag) or to the second --
    // wave-uniform, the split is a multiple of 32.
    int co = 32 * cb + l32;
    int cw = p.Cout, relu_f = p.relu;
    float *obase = sg.out;
    const float bv = (p.bias != nullptr && co < p.Cout) ? p.bias[co] : 0.f;
    if (MODE == 0 && p.sib_split > 0) {
        const bool second = 32 * cb >= p.sib_split;
        cw = second ? p.Cout - p.sib_split : p.sib_split;
        co = second ? co - p.sib_split : co;
        obase = second ? p.sib_out : sg.out;
        relu_f = second ? p.sib_relu : p.relu;
    }
    const bool co_ok = co < cw;
    const bool has_res = sg.res != nullptr;
    // (wave-uniform: readfirstlane makes that visible to the compiler -- the scalar-offset operands of the epilogue's buffer loads / stores
    // derived from it were otherwise materialised in VGPRs and every one of the 64 accesses of a lane wrapped in a waterfall loop)
    const unsigned crow = __builtin_amdgcn_readfirstlane((unsigned)cw * 4u);   // bytes of one output pixel (MODE 2: of the four pixels of a row)
    const size_t oaddr = reinterpret_cast<size_t>(obase);
    const unsigned olo = __builtin_amdgcn_readfirstlane((unsigned)oaddr), ohi = __builtin_amdgcn_readfirstlane((unsigned)(oaddr >> 32));
    const unsigned obytes = __builtin_amdgcn_readfirstlane((unsigned)sg.M * crow);
    const __amdgpu_buffer_rsrc_t orsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)ohi << 32) | olo), 0, (int)obytes, 0x00020000);
    if constexpr (MODE == 3) {
        // split-K: raw partial sums to the workspace [ksplit][m_total = m_tiles * 64][Cout]; bias / residual / ReLU in the reduce kernel
        const size_t paddr = reinterpret_cast<size_t>(p.partial + (long)kz * p.m_total * p.Cout);
        const unsigned plo = __builtin_amdgcn_readfirstlane((unsigned)paddr), phi = __builtin_amdgcn_readfirstlane((unsigned)(paddr >> 32));
        const __amdgpu_buffer_rsrc_t prsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)phi << 32) | plo), 0,
                                                                                (int)__builtin_amdgcn_readfirstlane((unsigned)p.m_total * crow), 0x00020000);
        const unsigned lane_p = co_ok ? (4u * (unsigned)lhalf * crow + 4u * (unsigned)co) : 0x80000000u;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const unsigned row0 = __builtin_amdgcn_readfirstlane((unsigned)(p0 + 32 * (NR == 2 ? i : wm)) * crow);
#pragma unroll
            for (int r = 0; r < 16; ++r)
                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(i == 0 ? acc0[r] : acc1[r]), prsrc, lane_p, row0 + (unsigned)((r & 3) + 8 * (r >> 2)) * crow, 0);
        }
        return;
    }
    if constexpr (MODE == 2) {
        // scatter epilogue. Row table: byte offset of output pixel (2h, 2w) of GEMM row p0 + t, or bit 31 beyond the map
        __syncthreads();                                               // every fragment read of the K walk is done: the A buffers are free
        unsigned *rowoff = reinterpret_cast<unsigned *>(smem_raw);
        const unsigned cpix = crow >> 2;                               // bytes of one output pixel: C floats
        if (tid < C1_BM) {
            const long pp = p0 + tid;
            unsigned o = 0x80000000u;
            if (pp < sg.M) {
                const int n = (int)(pp / HoWo);
                const int rem = (int)(pp - (long)n * HoWo);
                const int h = rem / sg.Wo, w = rem - h * sg.Wo;
                o = (unsigned)((n * 2 * sg.Ho + 2 * h) * 2 * sg.Wo + 2 * w) * cpix;
            }
            rowoff[tid] = o;
        }
        __syncthreads();
        const int cpl = p.Cout >> 2;                                   // C
        const int dydx = (32 * cb) / cpl, cc = co - dydx * cpl;        // wave-uniform (dy, dx); this lane's channel
        const unsigned lane_sc = co_ok ? (unsigned)((dydx >> 1) * 2 * sg.Wo + (dydx & 1)) * cpix + 4u * (unsigned)cc : 0x80000000u;
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            const int rb = 32 * (NR == 2 ? i : wm) + 4 * lhalf;
#pragma unroll
            for (int k4 = 0; k4 < 4; ++k4) {
                const uintx4 ro = *reinterpret_cast<const uintx4 *>(rowoff + rb + 8 * k4);   // rows rb + 8 k4 + {0..3}
                const unsigned rr4[4] = {ro.x, ro.y, ro.z, ro.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = 4 * k4 + j;
                    float v = i == 0 ? acc0[r] : acc1[r];
                    if (p.bias != nullptr) v = v + bv;
                    if (p.relu) v = fmaxf(v, 0.f);
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orsrc, (rr4[j] + lane_sc) | ((rr4[j] | lane_sc) & 0x80000000u), 0, 0);   // (bit 31 of either part: dropped)
                }
            }
        }
        return;
    }
    const unsigned lane_off = co_ok ? (4u * (unsigned)lhalf * crow + 4u * (unsigned)co) : 0x80000000u;
    const size_t raddr = reinterpret_cast<size_t>(has_res ? sg.res : sg.out);
    const unsigned rlo = __builtin_amdgcn_readfirstlane((unsigned)raddr), rhi = __builtin_amdgcn_readfirstlane((unsigned)(raddr >> 32));
    const int Hr = sg.Ho >> 1, Wr = sg.Wo >> 1;
    const unsigned rbytes = __builtin_amdgcn_readfirstlane(RESUP ? (unsigned)(sg.N * Hr * Wr) * crow : obytes);
    const __amdgpu_buffer_rsrc_t rrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)rhi << 32) | rlo), 0, (int)rbytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        const long pb0 = p0 + 32 * (NR == 2 ? i : wm);                 // first of the 32 consecutive output pixels of this block (wave-uniform)
        const unsigned row0 = __builtin_amdgcn_readfirstlane((unsigned)pb0 * crow);
        float rr[16];
        if (has_res) {
            if (RESUP && (sg.Wo & 31) == 0) {
                // Wo % 32 == 0 (every FPN level of the workloads): the 32 rows lie in one image row, the half-resolution source is one
                // base + (column >> 1) -- no division per row; the lane's row half (4 lhalf) shifts the source column by 2 lhalf
                const long pb = pb0 < sg.M ? pb0 : 0;
                const int n_b = (int)(pb / HoWo);
                const int rem_b = (int)(pb - (long)n_b * HoWo);
                const int h_b = rem_b / sg.Wo, w_b = rem_b - h_b * sg.Wo;      // w_b: multiple of 32
                const unsigned rb = __builtin_amdgcn_readfirstlane((unsigned)(((long)n_b * Hr + (h_b >> 1)) * Wr + (w_b >> 1)) * crow);
                const unsigned lane_r = co_ok ? (2u * (unsigned)lhalf * crow + 4u * (unsigned)co) : 0x80000000u;
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    rr[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, pb0 < sg.M ? lane_r : 0x80000000u,
                                                                                  rb + (unsigned)(((r & 3) + 8 * (r >> 2)) >> 1) * crow, 0));
            } else if (RESUP) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {   // general decomposition, one row at a time
                    long pp = pb0 + 4 * lhalf + (r & 3) + 8 * (r >> 2);
                    const bool ok = pp < sg.M && co_ok;
                    pp = pp < sg.M ? pp : sg.M - 1;
                    const int n = (int)(pp / HoWo);
                    const int rem = (int)(pp - (long)n * HoWo);
                    const int h = rem / sg.Wo, w = rem - h * sg.Wo;
                    const unsigned ri = (unsigned)(((long)n * Hr + (h >> 1)) * Wr + (w >> 1));
                    rr[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, ok ? ri * crow + 4u * (unsigned)co : 0x80000000u, 0, 0));
                }
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    rr[r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rrsrc, lane_off, row0 + (unsigned)((r & 3) + 8 * (r >> 2)) * crow, 0));
            }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = i == 0 ? acc0[r] : acc1[r];
            if (p.bias != nullptr) v = v + bv;
            if (has_res) v = v + rr[r];
            if (relu_f) v = fmaxf(v, 0.f);
            __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), orsrc, lane_off, row0 + (unsigned)((r & 3) + 8 * (r >> 2)) * crow, 0);
        }
    }
}

// development knob: 0 auto, 64 / 128 forced BN
static int g_c1_bn = 0;
extern "C" void upsnet_conv1x1_tuning(int bn) { g_c1_bn = bn; }

// mode: 0 plain, 1 residual through a nearest x2 upsampling, 2 transposed-convolution scatter (p.Cout = 4 C columns), 3 split-K (p.ksplit
// workgroups per tile, raw partial sums to p.partial; the caller reduces)
static int conv1x1_frag_launch(hipStream_t st, ConvParams &p, int mode)
{
    const int Cout = p.Cout;
    p.seg[0].tile_start = 0;
    p.m_tiles = (int)((p.seg[0].M + C1_BM - 1) / C1_BM);
    // BN = 128 halves the A traffic per output and doubles the MFMAs per LDS fragment; BN = 64 for narrow layers and for maps whose
    // 128-wide tiling would leave CUs idle (fewer than 2 workgroups per CU)
    int bn = g_c1_bn;
    if (!bn) bn = (Cout > 64 && (long)p.m_tiles * ((Cout + 127) / 128) >= 512) ? 128 : 64;
    if (Cout <= 64) bn = 64;
    p.n_tiles = (Cout + bn - 1) / bn;
    // (no static LDS; beyond the kernel's own 16 KiB only the padding of a residency cap, residency.h -- 4 workgroups per CU by registers)
    const size_t smem = res_dynamic_lds(RES_CONV1X1_FRAG, 0, (size_t)2 * 8 * C1_BM * 16);
    static std::atomic<unsigned long long> attr_dev{0};
#define C1_ATTR(NW, MODE) UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&conv1x1_frag_f32_kernel<NW, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, res_max_dynamic(0)))
    UPS_ONCE_PER_DEVICE(attr_dev, C1_ATTR(4, 0); C1_ATTR(4, 1); C1_ATTR(4, 2); C1_ATTR(4, 3); C1_ATTR(2, 0); C1_ATTR(2, 1); C1_ATTR(2, 2); C1_ATTR(2, 3));
#undef C1_ATTR
    p.m_total = (long)p.m_tiles * C1_BM;
    const int grid = 8 * ((p.m_tiles + 7) / 8) * p.n_tiles * (mode == 3 ? p.ksplit : 1);
#define C1_LAUNCH(NW, MODE) hipLaunchKernelGGL((conv1x1_frag_f32_kernel<NW, MODE>), dim3(grid), dim3(256), smem, st, p)
    if (bn == 128) { if (mode == 3) C1_LAUNCH(4, 3); else if (mode == 2) C1_LAUNCH(4, 2); else if (mode == 1) C1_LAUNCH(4, 1); else C1_LAUNCH(4, 0); }
    else { if (mode == 3) C1_LAUNCH(2, 3); else if (mode == 2) C1_LAUNCH(2, 2); else if (mode == 1) C1_LAUNCH(2, 1); else C1_LAUNCH(2, 0); }
#undef C1_LAUNCH
    UPS_CHECK_LAUNCH("conv1x1_frag_f32_kernel");
    ups_set_form("conv1x1_frag<%d,%d>", bn == 128 ? 4 : 2, mode);
    return 0;
}

/* out = relu?(conv1x1(x, w; stride) + bias + residual). x [N,H,W,Cin] NHWC, out [N,Ho,Wo,Cout] NHWC, residual like out, or -- with
 * residual_up -- [N,Ho/2,Wo/2,Cout] read through a nearest x2 upsampling. wpack: upsnet_dcn_pack_weight(weight, cout, cin, 1, 1). */
extern "C" int upsnet_conv1x1_frag_nhwc_f32(void *stream, const float *x, const float *residual, float *out, int batch, int height,
                                            int width, int Cin, const float *wpack, const float *bias, int Cout, int stride, int relu,
                                            int residual_up)
{
    const float *xs[1] = {x}, *rs[1] = {residual};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    const int ldw = (Cout + 31) / 32 * 32;
    int rc = conv_fill(p, "conv1x1_frag_nhwc_f32", 1, xs, residual ? rs : nullptr, nullptr, nullptr, os, nb, hh, ww, Cin, Cout, wpack, ldw, bias,
                       1, 1, stride, 0, 1, relu);
    if (rc) return rc;
    UPS_REQUIRE((long)batch * height * width * Cin < (1L << 29), "conv1x1_frag_nhwc_f32: feature map exceeds 2 GiB; split the batch");
    UPS_REQUIRE((long)p.seg[0].M * Cout < (1L << 29), "conv1x1_frag_nhwc_f32: output exceeds 2 GiB; split the batch");
    if (residual_up) {
        UPS_REQUIRE(residual, "conv1x1_frag_nhwc_f32: residual_up without a residual");
        UPS_REQUIRE(p.seg[0].Ho % 2 == 0 && p.seg[0].Wo % 2 == 0, "conv1x1_frag_nhwc_f32: residual_up needs even output dims");
    }
    return conv1x1_frag_launch((hipStream_t)stream, p, residual_up ? 1 : 0);
}

/* The same convolution with the K walk of every tile split over `ksplit` workgroups (MODE 3) + the shared reduce / epilogue kernel:
 * for maps whose tile count does not fill the 256 CUs evenly (a workgroup of this kernel keeps all four SIMDs of a CU at the MFMA rate,
 * so a launch takes max-workgroups-per-CU x one workgroup's K walk: 264 tiles = 2 walks, 264 x 4 quarter walks = 5 quarters).
 * workspace: upsnet_conv1x1_splitk_workspace_bytes(batch, Ho, Wo, Cout, ksplit) bytes. No residual_up. */
extern "C" size_t upsnet_conv1x1_splitk_workspace_bytes(int batch, int out_height, int out_width, int Cout, int ksplit)
{
    const long M = (long)batch * out_height * out_width;
    return (size_t)ksplit * ((M + C1_BM - 1) / C1_BM * C1_BM) * Cout * sizeof(float);
}

extern "C" int upsnet_conv1x1_frag_nhwc_f32_splitk(void *stream, const float *x, const float *residual, float *out, int batch, int height,
                                                   int width, int Cin, const float *wpack, const float *bias, int Cout, int stride, int relu,
                                                   int ksplit, void *workspace)
{
    const float *xs[1] = {x}, *rs[1] = {residual};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    const int ldw = (Cout + 31) / 32 * 32;
    int rc = conv_fill(p, "conv1x1_frag_nhwc_f32_splitk", 1, xs, residual ? rs : nullptr, nullptr, nullptr, os, nb, hh, ww, Cin, Cout, wpack, ldw,
                       bias, 1, 1, stride, 0, 1, relu);
    if (rc) return rc;
    const int nsl = Cin / 32;
    UPS_REQUIRE(workspace && ksplit >= 2 && ksplit <= 16, "conv1x1_frag_nhwc_f32_splitk: ksplit must be 2..16 and a workspace given");
    UPS_REQUIRE(((nsl + ksplit - 1) / ksplit) * (ksplit - 1) < nsl, "conv1x1_frag_nhwc_f32_splitk: %d K steps cannot be split %d ways", nsl, ksplit);
    UPS_REQUIRE((long)batch * height * width * Cin < (1L << 29), "conv1x1_frag_nhwc_f32_splitk: feature map exceeds 2 GiB; split the batch");
    UPS_REQUIRE((long)(p.seg[0].M + C1_BM) * Cout < (1L << 29), "conv1x1_frag_nhwc_f32_splitk: output exceeds 2 GiB; split the batch");
    p.ksplit = ksplit;
    p.partial = (float *)workspace;
    rc = conv1x1_frag_launch((hipStream_t)stream, p, 3);
    if (rc) return rc;
    return conv_splitk_reduce((hipStream_t)stream, p.partial, ksplit, p.m_total, p.seg[0].M, Cout, bias, residual, relu, out);
}

/* Two 1x1 convolutions of the SAME input in one launch (conv1 and the projection shortcut of a stage's first bottleneck, resnet.py:53-100):
 * out_a [N,Ho,Wo,cout_a] = relu_a?(conv(x; rows [0, cout_a) of the weight) + bias), out_b [N,Ho,Wo,cout_b] likewise from the remaining rows.
 * wpack: upsnet_dcn_pack_weight of the concatenated [cout_a + cout_b, Cin, 1, 1] weight; bias: the two biases concatenated (or NULL);
 * cout_a % 32 == 0. Every output element is computed exactly as in a launch of its own layer (bit-identical). */
extern "C" int upsnet_conv1x1_siblings_nhwc_f32(void *stream, const float *x, float *out_a, float *out_b, int batch, int height, int width,
                                                int Cin, const float *wpack, const float *bias, int cout_a, int cout_b, int stride, int relu_a,
                                                int relu_b)
{
    UPS_REQUIRE(out_a && out_b && cout_a > 0 && cout_b > 0 && cout_a % 32 == 0, "conv1x1_siblings_nhwc_f32: two outputs, cout_a %% 32 == 0 (got %d, %d)", cout_a, cout_b);
    const int Cout = cout_a + cout_b;
    const float *xs[1] = {x};
    float *os[1] = {out_a};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    const int ldw = (Cout + 31) / 32 * 32;
    int rc = conv_fill(p, "conv1x1_siblings_nhwc_f32", 1, xs, nullptr, nullptr, nullptr, os, nb, hh, ww, Cin, Cout, wpack, ldw, bias, 1, 1, stride, 0, 1, relu_a);
    if (rc) return rc;
    UPS_REQUIRE((long)batch * height * width * Cin < (1L << 29), "conv1x1_siblings_nhwc_f32: feature map exceeds 2 GiB; split the batch");
    // (the output descriptors of the epilogue carry 32-bit byte counts: rows x row bytes of the wider of the two outputs)
    UPS_REQUIRE((long)(p.seg[0].M + C1_BM) * (cout_a > cout_b ? cout_a : cout_b) < (1L << 29), "conv1x1_siblings_nhwc_f32: output exceeds 2 GiB; split the batch");
    p.sib_split = cout_a; p.sib_relu = relu_b; p.sib_out = out_b;
    rc = conv1x1_frag_launch((hipStream_t)stream, p, 0);
    if (rc == 0) ups_set_form("conv1x1_siblings<%d+%d>", cout_a, cout_b);
    return rc;
}

/* ConvTranspose2d(kernel 2, stride 2, pad 0) (+ bias, + ReLU) on the same kernel (MODE 2): x [N,H,W,Cin] NHWC -> out [N,2H,2W,Cout] NHWC.
 * wpack: upsnet_dcn_pack_weight of the [4 Cout, Cin, 1, 1] matrix whose rows are (dy, dx, co); bias4: the bias repeated for the four
 * (dy, dx) -- [4 Cout] -- or NULL. Cout % 32 == 0, Cin % 32 == 0. Reference: the mask head's upsampling layer, upsnet/models/rcnn.py:132-133. */
extern "C" int upsnet_deconv2x2_frag_nhwc_f32(void *stream, const float *x, float *out, int batch, int height, int width, int Cin,
                                              const float *wpack, const float *bias4, int Cout, int relu)
{
    UPS_REQUIRE(Cout > 0 && Cout % 32 == 0, "deconv2x2_frag_nhwc_f32: Cout must be a multiple of 32");
    const float *xs[1] = {x};
    float *os[1] = {out};
    const int nb[1] = {batch}, hh[1] = {height}, ww[1] = {width};
    ConvParams p;
    int rc = conv_fill(p, "deconv2x2_frag_nhwc_f32", 1, xs, nullptr, nullptr, nullptr, os, nb, hh, ww, Cin, 4 * Cout, wpack, 4 * Cout, bias4,
                       1, 1, 1, 0, 1, relu);
    if (rc) return rc;
    UPS_REQUIRE((long)batch * height * width * Cin < (1L << 29), "deconv2x2_frag_nhwc_f32: feature map exceeds 2 GiB; split the batch");
    UPS_REQUIRE((long)p.seg[0].M * 4 * Cout < (1L << 29), "deconv2x2_frag_nhwc_f32: output exceeds 2 GiB; split the batch");
    return conv1x1_frag_launch((hipStream_t)stream, p, 2);
}
