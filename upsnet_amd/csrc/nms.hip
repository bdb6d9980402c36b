// nms.hip -- hard / soft NMS for gfx950.
//
// Reference: upsnet/nms/gpu_nms.pyx:23-38 (host argsort + _nms), upsnet/nms/nms_kernel.cu:30-150
// (64x64 IoU bitmask tiles on the GPU, mask copied back, greedy scan on the HOST, cudaMalloc/Free per
// call), upsnet/nms/cpu_nms.pyx:91-196 (soft-NMS, host only).
//
// MI355X design: the whole thing stays on the device and is batched over P independent problems
// (all RPN levels / all classes at once):
//   1. nms_sort_kernel  : one workgroup per problem, bitonic sort of unique 64-bit keys
//                         (score bits << 32 | index) in LDS -> visiting order (score desc, index desc),
//                         i.e. the pinned meaning of scores.argsort()[::-1].
//   2. nms_mask_kernel  : 64-lane workgroups = one wavefront per 64x64 tile (upper triangle only),
//                         column boxes staged in LDS, one u64 suppression word per (row, tile).
//   3. nms_scan_kernel  : ONE wavefront per problem does the greedy scan: 64 candidates at a time are
//                         resolved in registers with ctz/readlane on the diagonal tile, then every lane
//                         ORs its own suppression words for the kept rows (coalesced row reads).
// Decisions use the reference's fp32 expression order without FMA -> keep lists are bit-exact.
#include <stdlib.h>

#include "common.h"
#include "soft_nms_trips.h"
#include "sort.h"
#include "upsnet_hip.h"

typedef unsigned long long u64;

__device__ static inline u64 shfl64(u64 v, int src)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
    lo = __shfl(lo, src, 64);
    hi = __shfl(hi, src, 64);
    return ((u64)hi << 32) | lo;
}

// tie_mode 0: equal scores -> higher index first; 1: lower index first.
__global__ void __launch_bounds__(1024)
nms_sort_kernel(const float *__restrict__ boxes, const float *__restrict__ scores, const int *__restrict__ counts,
                const int nmax, const int M, const int tie_mode, float4 *__restrict__ sorted_boxes,
                int *__restrict__ order)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64 *keys = reinterpret_cast<u64 *>(smem_raw);
    const int p = blockIdx.x, tid = threadIdx.x, bd = blockDim.x;
    const int n = min(counts[p], nmax);
    // sort only as many keys as this problem holds (the class-agnostic selection reserves 8192 slots and usually fills ~100:
    // 55 barrier-separated stages instead of 91)
    int Mp = 64;
    while (Mp < n) Mp <<= 1;
    Mp = min(Mp, M);
    for (int i = tid; i < Mp; i += bd)
        keys[i] = i < n ? ups_make_key(scores[(long)p * nmax + i], (unsigned)i, tie_mode) : 0ULL;
    if (Mp <= 128) ups_block_rank_sort_desc(keys, n, Mp);   // (unique, non-zero keys; small sets only, see sort.h)
    else ups_block_sort_desc(keys, Mp);
    const float4 *b4 = reinterpret_cast<const float4 *>(boxes) + (long)p * nmax;
    for (int i = tid; i < n; i += bd) {
        const int idx = (int)ups_key_index(keys[i], tie_mode);
        order[(long)p * nmax + i] = idx;
        sorted_boxes[(long)p * nmax + i] = b4[idx];
    }
}

// diagT[p][c]: for sorted box c, the 64-bit word of the boxes of ITS OWN 64-block that suppress it (bit j: box 64 (c/64) + j, j < c % 64,
// overlaps c above the threshold) -- the transpose of the diagonal tile, which is what the scan needs to resolve a block in parallel.
__global__ void __launch_bounds__(64)
nms_mask_kernel(const float4 *__restrict__ sboxes, const int *__restrict__ counts, const int nmax, const int CB,
                const float thresh, const int ge, u64 *__restrict__ mask, u64 *__restrict__ diagT)
{
    const int p = blockIdx.z;
    const int n = min(counts[p], nmax);
    const int row_start = blockIdx.y, col_start = blockIdx.x;
    if (row_start * 64 >= n || col_start * 64 >= n || col_start < row_start) return;
    const int row_size = min(n - row_start * 64, 64), col_size = min(n - col_start * 64, 64);
    __shared__ float4 cb[64];
    const int tid = threadIdx.x;
    if (tid < col_size) cb[tid] = sboxes[(long)p * nmax + col_start * 64 + tid];
    __syncthreads();
    const bool row_ok = tid < row_size;
    const int cur = row_start * 64 + tid;
    const float4 a = sboxes[(long)p * nmax + (row_ok ? cur : row_start * 64)];
    u64 t = 0;
    if (row_start != col_start) {
        if (row_ok) {
            for (int i = 0; i < col_size; ++i) {
                const float4 b = cb[i];
                const float ov = ups_iou(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
                if (ge ? ov >= thresh : ov > thresh) t |= 1ULL << i;   // nms_kernel.cu:73-80 is ">", cpu_nms.pyx:77 ">="
            }
            mask[((long)p * nmax + cur) * CB + col_start] = t;
        }
        return;
    }
    // diagonal tile: uniform loop over the columns, so that one ballot per column yields the column's (transposed) word
    u64 tw = 0;
    for (int i = 0; i < col_size; ++i) {
        const float4 b = cb[i];
        const float ov = ups_iou(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w);
        const bool hit = row_ok && i > tid && (ge ? ov >= thresh : ov > thresh);
        if (hit) t |= 1ULL << i;
        const u64 colw = __ballot(hit);
        if (tid == i) tw = colw;
    }
    if (row_ok) {
        mask[((long)p * nmax + cur) * CB + col_start] = t;
        diagT[(long)p * nmax + cur] = tw;
    }
}

// uniform-lane read of a 64-bit value: v_readlane (scalar path, a few cycles) instead of a shuffle through the
// LDS crossbar; `src` must be wave-uniform.
__device__ static inline u64 readlane64(u64 v, int src)
{
    const int s = __builtin_amdgcn_readfirstlane(src);
    const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)v, s), hi = __builtin_amdgcn_readlane((int)(unsigned)(v >> 32), s);
    return ((u64)hi << 32) | lo;
}

#define NMS_SCAN_T 256
#define NMS_LDS_ROWS 1024   // problems up to this many boxes keep their whole suppression mask in LDS (<= 128 KiB)

// One workgroup per problem. All threads stage the mask rows into LDS (problems of <= 1024 boxes; row pitch = a power of two,
// no division), then wave 0 walks the 64-blocks in order:
//   * a block is resolved IN PARALLEL from the transposed diagonal words (nms_mask_kernel): kept = alive; repeat kept' = alive &
//     ~{ c : T_c & kept & (bits below c) != 0 } until nothing changes. After t rounds the first t+1 live boxes of the block are
//     final, and a fixed point satisfies the greedy recurrence "c is kept iff it is alive and no kept predecessor suppresses it"
//     for every c, whose solution is unique -- so the result IS the sequential scan of nms_kernel.cu:130-146, typically after 2-5
//     rounds of ~6 instructions instead of up to 64 dependent ctz / readlane / and trips;
//   * the suppression words of the kept rows are ORed into the per-column-block state by all 64 lanes: lane = (column block w,
//     phase tq) reads the rows 4k + tq of the block (16 independent LDS reads), two xor-shuffles combine the four phases.
// r05's scan (one dependent LDS read per kept row, sequential diagonal) took 120-140 us for 1000 boxes; this one ~15.
// (<= 128 registers: a scan wave must fit beside the three 124-register waves per SIMD of the deformable kernel it runs next to)
typedef unsigned nms_uintx2 __attribute__((ext_vector_type(2)));

template <bool LDS>
__global__ void __launch_bounds__(NMS_SCAN_T) __attribute__((amdgpu_waves_per_eu(4, 4)))
nms_scan_kernel(const u64 *__restrict__ mask, const u64 *__restrict__ diagT, const int *__restrict__ order,
                const int *__restrict__ counts, const uint8_t *__restrict__ pre_removed, const int nmax, const int CB,
                int *__restrict__ keep_idx, int *__restrict__ keep_cnt)
{
    constexpr int use_lds = LDS ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    u64 *smask = reinterpret_cast<u64 *>(smem_raw);
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = min(counts[p], nmax);
    const int nb = (n + 63) >> 6;
    const u64 *mp = mask + (long)p * nmax * CB;
    int lg = 0;
    while ((1 << lg) < nb) ++lg;
    const int pitch = use_lds ? (1 << lg) : CB;          // u64 words per mask row as the scan reads it
    if (use_lds) {
        // only words (row i, column block >= i/64) were produced by nms_mask_kernel; copy exactly those
        for (int idx = tid; idx < (n << lg); idx += (int)blockDim.x) {
            const int i = idx >> lg, cb = idx & (pitch - 1);
            if (cb < nb && cb >= (i >> 6)) smask[idx] = mp[(long)i * CB + cb];
        }
        __syncthreads();
    }
    if (tid >= 64) return;
    const int lane = tid;
    // mask rows of this problem: LDS copy, or buffer loads (one lane offset per block + a scalar row offset per load: no 64-bit
    // address arithmetic, and a column block outside (b, nb) is an out-of-range offset that reads 0)
    const size_t maddr = reinterpret_cast<size_t>(mp);
    const unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)maddr), mhi = __builtin_amdgcn_readfirstlane((unsigned)(maddr >> 32));
    const __amdgpu_buffer_rsrc_t mrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)mhi << 32) | mlo), 0,
                                                                           (int)((unsigned)nmax * (unsigned)CB * 8u), 0x00020000);
#define NMS_ROWWORD(ROW_UNIFORM, LANE_ROW, W, OK, DST)                                                                     \
    if (LDS) { DST = (OK) ? smask[(long)((ROW_UNIFORM) + (LANE_ROW)) * pitch + (W)] : 0ULL; }                              \
    else {                                                                                                                 \
        const nms_uintx2 v_ = __builtin_amdgcn_raw_buffer_load_b64(mrsrc, (OK) ? (unsigned)((LANE_ROW) * pitch + (W)) * 8u : 0x80000000u, \
                                                                   (unsigned)(ROW_UNIFORM) * (unsigned)pitch * 8u, 0);     \
        DST = ((u64)v_.y << 32) | v_.x;                                                                                    \
    }
    const int *ord = order ? order + (long)p * nmax : nullptr;
    const u64 below = (1ULL << lane) - 1ULL;
    int nkeep = 0;
    // suppression state: lane w holds the words of column blocks w and w + 64 (nmax <= 8192)
    u64 remv0 = 0, remv1 = 0;
    const int wq = lane & 15, tq = lane >> 4;            // OR phase: column block slot, row phase
    // Everything a block needs from memory is STATIC (the sort order, the pre-removed flags, the transposed diagonal words and the
    // mask rows of its 64 boxes for the next 16 column blocks): none of it depends on the scan state, only its USE does (which rows
    // are ORed in). So the loads of block b+1 are issued before block b is resolved (two statically named register sets, the loop
    // unrolled by two: no copies), and the kept bits select among already loaded rows. r07 issued them on demand: three dependent
    // memory latencies per block (order -> pre_removed; diagonal; the kept rows), 16 blocks in a row = 50-90 us for 1000 boxes.
#define NMS_SET(S) int oi_##S = 0; bool pre_##S = false; u64 tw_##S = 0; u64 r_##S[16];
#define NMS_FETCH(S, B)                                                                                                    \
    {                                                                                                                      \
        const int i_ = (B) * 64 + lane;                                                                                    \
        const bool v_ = i_ < n;                                                                                            \
        oi_##S = v_ ? (ord ? ord[i_] : i_) : 0;                                                                            \
        pre_##S = v_ && pre_removed && pre_removed[(long)p * nmax + oi_##S];                                               \
        tw_##S = v_ ? diagT[(long)p * nmax + i_] : 0;      /* boxes of this block that suppress box i */                   \
        const int w_ = (((B) + 1) & ~15) + wq;                                                                             \
        _Pragma("unroll") for (int k = 0; k < 16; ++k)                                                                     \
            NMS_ROWWORD((B) * 64 + 4 * k, tq, w_, w_ > (B) && w_ < nb, r_##S[k])                                           \
    }
#define NMS_BLOCK(S, B)                                                                                                    \
    {                                                                                                                      \
        const int b = (B);                                                                                                 \
        const u64 cur = readlane64(b < 64 ? remv0 : remv1, b & 63);                                                        \
        const bool valid = b * 64 + lane < n;                                                                              \
        const u64 alive = ~cur & __ballot(valid) & ~__ballot(pre_##S);                                                     \
        u64 kept = alive;                                                                                                  \
        for (;;) {                                                                                                         \
            const u64 nk = alive & ~__ballot((tw_##S & kept & below) != 0);                                                \
            if (nk == kept) break;                                                                                         \
            kept = nk;                                                                                                     \
        }                                                                                                                  \
        if ((kept >> lane) & 1ULL)                                                                                         \
            keep_idx[(long)p * nmax + nkeep + __builtin_popcountll(kept & below)] = oi_##S;                                \
        nkeep += __builtin_popcountll(kept);                                                                               \
        /* OR the rows of the kept boxes into the state of the later column blocks, 16 column blocks per pass; the first pass */ \
        /* from the prefetched rows, further passes (more than 1024 boxes) on demand */                                    \
        for (int w0 = (b + 1) & ~15; w0 < nb; w0 += 16) {                                                                  \
            const int w = w0 + wq;                                                                                         \
            u64 acc = 0;                                                                                                   \
            if (w0 == ((b + 1) & ~15)) {                                                                                   \
                _Pragma("unroll") for (int k = 0; k < 16; ++k)                                                             \
                    if ((kept >> (4 * k + tq)) & 1ULL) acc |= r_##S[k];                                                    \
            } else if (w > b && w < nb) {                                                                                  \
                _Pragma("unroll 4") for (int k = 0; k < 16; ++k) {                                                         \
                    u64 word_;                                                                                             \
                    NMS_ROWWORD(b * 64 + 4 * k, tq, w, true, word_)                                                        \
                    if ((kept >> (4 * k + tq)) & 1ULL) acc |= word_;                                                       \
                }                                                                                                          \
            }                                                                                                              \
            acc |= shfl64(acc, lane ^ 16);                                                                                 \
            acc |= shfl64(acc, lane ^ 32);                                                                                 \
            /* lane `wq` of each 16-group now holds the OR for column block w0 + wq; hand it to the lane that owns that block */ \
            const u64 mine0 = shfl64(acc, lane & 15);               /* value for column block w0 + (lane & 15) */          \
            if (lane >= (w0 & 63) && lane < (w0 & 63) + 16) {                                                              \
                if (w0 < 64) remv0 |= mine0; else remv1 |= mine0;                                                          \
            }                                                                                                              \
        }                                                                                                                  \
    }
    NMS_SET(A)
    NMS_SET(B)
    if (nb > 0) NMS_FETCH(A, 0)
    for (int b0 = 0; b0 < nb; b0 += 2) {
        if (b0 + 1 < nb) NMS_FETCH(B, b0 + 1)
        NMS_BLOCK(A, b0)
        if (b0 + 1 >= nb) break;
        if (b0 + 2 < nb) NMS_FETCH(A, b0 + 2)
        NMS_BLOCK(B, b0 + 1)
    }
#undef NMS_SET
#undef NMS_ROWWORD
#undef NMS_FETCH
#undef NMS_BLOCK
    if (lane == 0) keep_cnt[p] = nkeep;
}

// ---------------------------------------------------------------------------------------------
// r08: the scan for problems of <= 1024 boxes (every RPN level, every class) in ROW layout, fully unrolled over the <= 16 blocks.
// What is sequential in greedy NMS is one 64-bit word per block: cur_b = OR over the kept rows of all earlier blocks of their
// word for column block b. The r05-r07 scan pushed the kept rows of block j eagerly into the state of ALL later column blocks with
// lane = (column block, row phase): 16 guarded 64-bit ORs on freshly loaded words, three 64-bit LDS-crossbar shuffles and a
// readlane per block, ~500 dependent instructions of ONE wave = 2.7 us per block, 43 us for 1000 boxes (a lone wave issues an
// instruction every ~5 cycles). Here lane = ROW: lane l of block j owns row 64 j + l, holds that row's words for the later column
// blocks (one contiguous 128-byte run: eight 16-byte buffer loads, prefetched one block ahead; scalars two blocks ahead), and ORs
// them into its private accumulators acc[c] if it is kept -- one exec-masked v_or per word, no cross-lane traffic. Only when block c
// is reached is acc[c] reduced over the 64 lanes: four DPP steps inside each row of 16 (quad_perm x 2, row_half_mirror, row_mirror:
// OR is idempotent, so mirrors are as good as rotations) + four v_readlane per half = a SCALAR cur_c in ~25 instructions.
// The diagonal block is resolved by the same fixed point as before. ~100 instructions per block; keep lists are bit-identical.
__device__ static inline unsigned nms_row_or(unsigned v)
{
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1,0,3,2]
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v |= (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
    return v;
}

__device__ static inline u64 nms_wave_or(u64 v)    // OR over the 64 lanes, wave-uniform result
{
    const unsigned lo = nms_row_or((unsigned)v), hi = nms_row_or((unsigned)(v >> 32));
    const unsigned rl = __builtin_amdgcn_readlane((int)lo, 0) | __builtin_amdgcn_readlane((int)lo, 16) |
                        __builtin_amdgcn_readlane((int)lo, 32) | __builtin_amdgcn_readlane((int)lo, 48);
    const unsigned rh = __builtin_amdgcn_readlane((int)hi, 0) | __builtin_amdgcn_readlane((int)hi, 16) |
                        __builtin_amdgcn_readlane((int)hi, 32) | __builtin_amdgcn_readlane((int)hi, 48);
    return ((u64)rh << 32) | rl;
}

typedef unsigned nms_uintx4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
nms_scan16_kernel(const u64 *__restrict__ mask, const u64 *__restrict__ diagT, const int *__restrict__ order,
                  const int *__restrict__ counts, const uint8_t *__restrict__ pre_removed, const int nmax, const int CB,
                  int *__restrict__ keep_idx, int *__restrict__ keep_cnt)
{
    const int p = blockIdx.x, lane = threadIdx.x;
    const int n = min(counts[p], nmax);
    const int nb = (n + 63) >> 6;                       // <= 16 (the launcher guarantees nmax <= 1024)
    const int *ord = order ? order + (long)p * nmax : nullptr;
    const u64 *dg = diagT + (long)p * nmax;
    const uint8_t *prm = pre_removed ? pre_removed + (long)p * nmax : nullptr;
    int *kout = keep_idx + (long)p * nmax;
    const u64 below = (1ULL << lane) - 1ULL;
    const size_t maddr = reinterpret_cast<size_t>(mask + (long)p * nmax * CB);
    const unsigned mlo = __builtin_amdgcn_readfirstlane((unsigned)maddr), mhi = __builtin_amdgcn_readfirstlane((unsigned)(maddr >> 32));
    // (rows 64 j + l >= nmax of the last block lie beyond the problem's mask: out of the descriptor's range, they read 0)
    const __amdgpu_buffer_rsrc_t mrsrc = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void *>(((size_t)mhi << 32) | mlo), 0,
                                                                           (int)((unsigned)nmax * (unsigned)CB * 8u), 0x00020000);
    const unsigned row_pitch = (unsigned)CB * 8u;
    u64 acc[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = 0;
    int oi[3];            // sort order of this lane's box in blocks j, j+1, j+2 (ring, index j % 3)
    bool pre[2];          // pre-removed flag, blocks j, j+1 (index j & 1)
    u64 tw[2];            // transposed diagonal word
    nms_uintx4 rw[2][8];  // the row's words for column blocks 2m, 2m+1 (m = 0..7); only m >= (j + 1) / 2 is loaded and used
#define S16_ORD(J) { const int i_ = (J) * 64 + lane; oi[(J) % 3] = i_ < n ? (ord ? ord[i_] : i_) : 0; }
#define S16_STATIC(J)                                                                                                      \
    {                                                                                                                      \
        const int i_ = (J) * 64 + lane;                                                                                    \
        const bool v_ = i_ < n;                                                                                            \
        pre[(J) & 1] = v_ && prm && prm[oi[(J) % 3]];                                                                      \
        tw[(J) & 1] = v_ ? dg[i_] : 0ULL;                                                                                  \
        const unsigned vo_ = (unsigned)i_ * row_pitch;                                                                     \
        _Pragma("unroll") for (int m = ((J) + 1) / 2; m < 8; ++m)                                                          \
            if (2 * m < CB) rw[(J) & 1][m] = __builtin_amdgcn_raw_buffer_load_b128(mrsrc, vo_ + 16u * (unsigned)m, 0, 0);  \
    }
    if (nb > 0) S16_ORD(0)
    if (nb > 1) S16_ORD(1)
    if (nb > 0) S16_STATIC(0)
    int nkeep = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j >= nb) continue;          // (wave-uniform; no `break`: the loop must keep its constant trip count to be unrolled)
        if (j + 2 < 16 && j + 2 < nb) S16_ORD(j + 2)
        if (j + 1 < 16 && j + 1 < nb) S16_STATIC(j + 1)
        const u64 cur = nms_wave_or(acc[j]);
        const bool valid = j * 64 + lane < n;
        const u64 alive = ~cur & __ballot(valid) & ~__ballot(pre[j & 1]);
        const u64 twj = tw[j & 1];
        u64 kept = alive;
        for (;;) {
            const u64 nk = alive & ~__ballot((twj & kept & below) != 0);
            if (nk == kept) break;
            kept = nk;
        }
        const bool mine = (kept >> lane) & 1ULL;
        if (mine) kout[nkeep + __builtin_popcountll(kept & below)] = oi[j % 3];
        nkeep += __builtin_popcountll(kept);
        if (mine) {
#pragma unroll
            for (int m = (j + 1) / 2; m < 8; ++m) {
                const nms_uintx4 w = rw[j & 1][m];
                if (2 * m > j) acc[2 * m] |= ((u64)w.y << 32) | w.x;
                acc[2 * m + 1] |= ((u64)w.w << 32) | w.z;
            }
        }
    }
#undef S16_ORD
#undef S16_STATIC
    if (lane == 0) keep_cnt[p] = nkeep;
}

static inline int next_pow2(int v) { int m = 64; while (m < v) m <<= 1; return m; }

struct NmsWs {
    float4 *sorted_boxes;
    int *order;
    u64 *diagT;
    u64 *mask;
};
static inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
static NmsWs nms_carve(void *ws, int P, int nmax)
{
    NmsWs w;
    unsigned char *b = (unsigned char *)ws;
    w.sorted_boxes = (float4 *)b; b += align256((size_t)P * nmax * sizeof(float4));
    w.order = (int *)b; b += align256((size_t)P * nmax * sizeof(int));
    w.diagT = (u64 *)b; b += align256((size_t)P * nmax * sizeof(u64));
    w.mask = (u64 *)b;
    return w;
}

extern "C" size_t upsnet_nms_workspace_bytes(int P, int nmax)
{
    if (P <= 0 || nmax <= 0) return 256;
    size_t CB = ((size_t)nmax + 63) / 64;
    return align256((size_t)P * nmax * sizeof(float4)) + align256((size_t)P * nmax * sizeof(int)) +
           align256((size_t)P * nmax * sizeof(u64)) + align256((size_t)P * nmax * CB * sizeof(u64)) + 256;
}

// development knob: 1 = stage the suppression mask in LDS (problems of <= 1024 boxes), 0 (default, or UPSNET_NMS_LDS unset) = read it from L2
static int g_nms_lds = (getenv("UPSNET_NMS_LDS") != nullptr && getenv("UPSNET_NMS_LDS")[0] == '1') ? 1 : 0;
static int g_nms_scan16 = (getenv("UPSNET_NMS_SCAN16") != nullptr && getenv("UPSNET_NMS_SCAN16")[0] == '0') ? 0 : 1;
// lds_staging: 0 = default (row-layout scan for <= 1024 boxes, L2 reads otherwise), 1 = LDS-staged mask (r05 form), 2 = the general
// scan for every size (r07 form)
extern "C" void upsnet_nms_tuning(int lds_staging) { g_nms_lds = lds_staging == 1 ? 1 : 0; g_nms_scan16 = lds_staging == 0 ? 1 : 0; }

// internal (proposal.hip, r11): the caller's own kernel has already written the visiting order -- `order` [P][nmax] (position -> input
// index) and `sorted_boxes` [P][nmax] -- into the workspace (its boxes arrive sorted by score: no second sort launch): views of those two
// arrays, and the mask + scan half of ups_nms_batched_impl.
void ups_nms_ws_views(void *workspace, int P, int nmax, float4 **sorted_boxes, int **order)
{
    NmsWs w = nms_carve(workspace, P, nmax);
    *sorted_boxes = w.sorted_boxes;
    *order = w.order;
}

static int nms_mask_scan(hipStream_t st, const NmsWs &w, const int *counts, const uint8_t *pre_removed, int P, int nmax, float thresh,
                         int *keep_idx, int *keep_cnt, int ge);

int ups_nms_batched_presorted_impl(hipStream_t st, const int *counts, const uint8_t *pre_removed, int P, int nmax, float thresh,
                                   int *keep_idx, int *keep_cnt, void *workspace, int ge)
{
    UPS_REQUIRE(counts && keep_idx && keep_cnt && workspace, "nms_batched_presorted: null pointer");
    UPS_REQUIRE(P > 0 && nmax > 0 && nmax <= 8192, "nms_batched_presorted: bad sizes P=%d nmax=%d", P, nmax);
    return nms_mask_scan(st, nms_carve(workspace, P, nmax), counts, pre_removed, P, nmax, thresh, keep_idx, keep_cnt, ge);
}

// internal: tie_mode-selectable version used by the proposal / detection pipelines
int ups_nms_batched_impl(hipStream_t st, const float *boxes, const float *scores, const int *counts,
                         const uint8_t *pre_removed, int P, int nmax, float thresh, int tie_mode, int *keep_idx,
                         int *keep_cnt, void *workspace, int ge)
{
    UPS_REQUIRE(boxes && scores && counts && keep_idx && keep_cnt && workspace, "nms_batched: null pointer");
    UPS_REQUIRE(P > 0 && nmax > 0, "nms_batched: bad sizes P=%d nmax=%d", P, nmax);
    UPS_REQUIRE(nmax <= 8192, "nms_batched: nmax=%d exceeds the 8192 boxes per problem supported", nmax);
    NmsWs w = nms_carve(workspace, P, nmax);
    const int M = next_pow2(nmax);
    hipLaunchKernelGGL(nms_sort_kernel, dim3(P), dim3(M < 1024 ? M : 1024), (size_t)M * sizeof(u64), st, boxes, scores,
                       counts, nmax, M, tie_mode, w.sorted_boxes, w.order);
    UPS_CHECK_LAUNCH("nms_sort_kernel");
    return nms_mask_scan(st, w, counts, pre_removed, P, nmax, thresh, keep_idx, keep_cnt, ge);
}

static int nms_mask_scan(hipStream_t st, const NmsWs &w, const int *counts, const uint8_t *pre_removed, int P, int nmax, float thresh,
                         int *keep_idx, int *keep_cnt, int ge)
{
    const int CB = (nmax + 63) / 64;
    hipLaunchKernelGGL(nms_mask_kernel, dim3(CB, CB, P), dim3(64), 0, st, w.sorted_boxes, counts, nmax, CB, thresh, ge, w.mask, w.diagT);
    UPS_CHECK_LAUNCH("nms_mask_kernel");
    // LDS staging of the mask (128 KiB for 1000 boxes) makes the scan ~20 % faster in isolation, but a workgroup that needs 128 KiB
    // cannot start on a CU that still hosts workgroups of the concurrently running semantic head (34 KiB each): inside the forward
    // the RPN scan took 383 us instead of 50 (profiles/r06_timeline_serial.txt). Default: read the kept rows from L2 (no LDS):
    // 215 us there, 139.5 -> 141.2 img/s, serial 8.09 -> 7.89 ms; UPSNET_NMS_LDS=1 restores the staging. (What remains is the wait
    // for a wave slot: the deformable kernel's workgroups hold 504 of the 512 VGPRs of a SIMD. s_setprio 3 on the chain kernels was
    // measured too: no effect -- they are not short of issue slots, they are waiting to be placed.)
    const int use_lds = g_nms_lds && nmax <= NMS_LDS_ROWS;
    int cbp = 1;
    while (cbp < CB) cbp <<= 1;
    const size_t scan_smem = use_lds ? (size_t)nmax * cbp * sizeof(u64) : 0;
    if (scan_smem > 64 * 1024) {
        static std::atomic<unsigned long long> attr_dev{0};
        UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&nms_scan_kernel<true>),
                                                                        hipFuncAttributeMaxDynamicSharedMemorySize, NMS_LDS_ROWS * (NMS_LDS_ROWS / 64) * 8)));
    }
    if (!use_lds && nmax <= 1024 && g_nms_scan16)
        hipLaunchKernelGGL(nms_scan16_kernel, dim3(P), dim3(64), 0, st, w.mask, w.diagT, w.order, counts, pre_removed, nmax, CB, keep_idx, keep_cnt);
    else if (use_lds)
        hipLaunchKernelGGL(nms_scan_kernel<true>, dim3(P), dim3(NMS_SCAN_T), scan_smem, st, w.mask, w.diagT, w.order, counts, pre_removed, nmax, CB,
                           keep_idx, keep_cnt);
    else
        hipLaunchKernelGGL(nms_scan_kernel<false>, dim3(P), dim3(64), 0, st, w.mask, w.diagT, w.order, counts, pre_removed, nmax, CB,
                           keep_idx, keep_cnt);
    UPS_CHECK_LAUNCH("nms_scan_kernel");
    return 0;
}

extern "C" int upsnet_nms_batched(void *stream, const float *boxes, const float *scores, const int *counts,
                                  const uint8_t *pre_removed, int P, int nmax, float thresh, int *keep_idx,
                                  int *keep_cnt, void *workspace)
{
    return ups_nms_batched_impl((hipStream_t)stream, boxes, scores, counts, pre_removed, P, nmax, thresh, 0, keep_idx,
                                keep_cnt, workspace, 0);
}

// cpu_nms semantics (cpu_nms.pyx:29-80) on the device: same visiting order and IoU expression, suppression at
// `ovr >= thresh` with the threshold a DOUBLE (a Python float in the reference's compiled module): the fp32 overlap is
// >= the double threshold iff it is >= the smallest fp32 number that is >= the threshold.
extern "C" int upsnet_cpu_nms_batched(void *stream, const float *boxes, const float *scores, const int *counts, int P, int nmax,
                                      double thresh, int *keep_idx, int *keep_cnt, void *workspace)
{
    float tf = (float)thresh;
    if ((double)tf < thresh) tf = nextafterf(tf, INFINITY);
    return ups_nms_batched_impl((hipStream_t)stream, boxes, scores, counts, nullptr, P, nmax, tf, 0, keep_idx, keep_cnt,
                                workspace, 1);
}

// ---------------------------------------------------------------------------------------------
// `_nms` drop-in: host pointers, boxes already sorted (gpu_nms.hpp:15).
__global__ void nms_pack_kernel(const float *__restrict__ boxes, int n, int dim, float4 *__restrict__ out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_float4(boxes[(long)i * dim], boxes[(long)i * dim + 1], boxes[(long)i * dim + 2],
                                    boxes[(long)i * dim + 3]);
}

extern "C" int upsnet_nms_host(int *keep_out, int *num_out, const float *boxes_host, int boxes_num, int boxes_dim,
                               float thresh, int device_id)
{
    UPS_REQUIRE(keep_out && num_out && (boxes_host || boxes_num == 0), "nms_host: null pointer");
    UPS_REQUIRE(boxes_dim >= 4, "nms_host: boxes_dim must be >= 4");
    *num_out = 0;
    if (boxes_num == 0) return 0;
    UPS_REQUIRE(boxes_num <= 8192, "nms_host: at most 8192 boxes supported (got %d)", boxes_num);
    int cur = 0;
    UPS_CHECK_HIP(hipGetDevice(&cur));
    if (cur != device_id) UPS_CHECK_HIP(hipSetDevice(device_id));
    const int n = boxes_num, CB = (n + 63) / 64;
    float *raw = nullptr; float4 *packed = nullptr; u64 *mask = nullptr, *diagT = nullptr; int *cnt = nullptr, *keep = nullptr, *kc = nullptr;
    UPS_CHECK_HIP(hipMalloc(&raw, (size_t)n * boxes_dim * sizeof(float)));
    UPS_CHECK_HIP(hipMalloc(&packed, (size_t)n * sizeof(float4)));
    UPS_CHECK_HIP(hipMalloc(&mask, (size_t)n * CB * sizeof(u64)));
    UPS_CHECK_HIP(hipMalloc(&diagT, (size_t)n * sizeof(u64)));
    UPS_CHECK_HIP(hipMalloc(&cnt, sizeof(int)));
    UPS_CHECK_HIP(hipMalloc(&keep, (size_t)n * sizeof(int)));
    UPS_CHECK_HIP(hipMalloc(&kc, sizeof(int)));
    int rc = 0;
    do {
        if (hipMemcpy(raw, boxes_host, (size_t)n * boxes_dim * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(cnt, &n, sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { rc = ups_set_error("nms_host: H2D copy failed"); break; }
        hipLaunchKernelGGL(nms_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, raw, n, boxes_dim, packed);
        hipLaunchKernelGGL(nms_mask_kernel, dim3(CB, CB, 1), dim3(64), 0, 0, packed, cnt, n, CB, thresh, 0, mask, diagT);
        hipLaunchKernelGGL(nms_scan_kernel<false>, dim3(1), dim3(64), 0, 0, mask, diagT, (const int *)nullptr, cnt, (const uint8_t *)nullptr,
                           n, CB, keep, kc);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { rc = ups_set_error("nms_host: launch failed: %s", hipGetErrorString(e)); break; }
        if (hipMemcpy(num_out, kc, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(keep_out, keep, (size_t)(*num_out) * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) {
            rc = ups_set_error("nms_host: D2H copy failed"); break;
        }
    } while (0);
    (void)hipFree(raw); (void)hipFree(packed); (void)hipFree(mask); (void)hipFree(diagT); (void)hipFree(cnt); (void)hipFree(keep); (void)hipFree(kc);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Soft-NMS (cpu_nms.pyx:91-196), batched: ONE workgroup per problem (RPN level / class), P problems per launch.
// The outer loop is sequential by definition; the trips (arg-max, swap, re-score, "swap with last" compaction) and their arithmetic
// are snms_lds_trips / snms_rescore of soft_nms_trips.h, shared with the soft detection selection (detect.hip).
//
// The state of a problem -- x1/y1/x2/y2/score/index as structure-of-arrays -- lives in LDS (28 bytes per box: 1024 boxes =
// 28 KiB, 4096 = 112 KiB of the CU's 160 KiB); problems up to 1024 boxes run on ONE wavefront (every "barrier" is free, ranks
// come from ballots), up to 4096 on four. A trip costs a few hundred cycles instead of the ~10 global-memory round trips of the
// r01 kernel (kept below for n > 4096).
template <int T>
__global__ void __launch_bounds__(T)
soft_nms_lds_kernel(float *__restrict__ boxes_g, int64_t *__restrict__ inds_g, const int *__restrict__ counts, const int nmax,
                    const int cap, const float sigma, const float Nt, const float threshold, const int method,
                    int *__restrict__ n_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ SnmsScratch<T> scratch;
    const SnmsState s = snms_carve(smem_raw, cap);
    const int p = blockIdx.x, tid = threadIdx.x;
    float *bg = boxes_g + (size_t)p * nmax * 5;
    int64_t *ig = inds_g + (size_t)p * nmax;
    const int n = counts ? min(counts[p], nmax) : nmax;
    for (int q = tid; q < n; q += T) {
        s.x1[q] = bg[q * 5 + 0]; s.y1[q] = bg[q * 5 + 1]; s.x2[q] = bg[q * 5 + 2]; s.y2[q] = bg[q * 5 + 3]; s.sc[q] = bg[q * 5 + 4];
        s.ind[q] = q;
    }
    __syncthreads();
    const int N = snms_lds_trips<T>(s, scratch, n, sigma, Nt, threshold, method);
    for (int q = tid; q < n; q += T) {
        bg[q * 5 + 0] = s.x1[q]; bg[q * 5 + 1] = s.y1[q]; bg[q * 5 + 2] = s.x2[q]; bg[q * 5 + 3] = s.y2[q]; bg[q * 5 + 4] = s.sc[q];
        ig[q] = s.ind[q];
    }
    if (tid == 0) n_out[p] = N;
}

// ---- global-memory form for problems beyond SNMS_LDS_MAX boxes (one workgroup of 1024 threads per problem)
#define SNMS_T 1024

__device__ static inline int block_excl_scan(int v, int *sh_wave, int *total)
{
    // exclusive prefix sum over the workgroup (blockDim.x == SNMS_T); returns this thread's offset
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { int y = __shfl_up(x, d, 64); if (lane >= d) x += y; }
    if (lane == 63) sh_wave[wave] = x;
    __syncthreads();
    if (wave == 0) {
        int s = lane < (SNMS_T / 64) ? sh_wave[lane] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { int y = __shfl_up(s, d, 64); if (lane >= d) s += y; }
        if (lane < (SNMS_T / 64)) sh_wave[lane] = s;  // inclusive over waves
    }
    __syncthreads();
    const int base = wave == 0 ? 0 : sh_wave[wave - 1];
    *total = sh_wave[SNMS_T / 64 - 1];
    __syncthreads();
    return base + x - v;
}

__global__ void __launch_bounds__(SNMS_T)
soft_nms_kernel(float *__restrict__ boxes, int64_t *__restrict__ inds, const int *__restrict__ counts, const int nmax,
                const float sigma, const float Nt, const float threshold, const int method, int *__restrict__ n_out,
                float *__restrict__ tmp_box, int64_t *__restrict__ tmp_ind, uint8_t *__restrict__ flag)
{
    {   // problem blockIdx.x: its slice of every buffer
        const size_t pb = blockIdx.x;
        boxes += pb * nmax * 5; inds += pb * nmax; n_out += pb;
        tmp_box += pb * nmax * 6; tmp_ind += pb * nmax * 2; flag += pb * nmax;
    }
    const int n = counts ? min(counts[blockIdx.x], nmax) : nmax;
    __shared__ float s_val[SNMS_T / 64];
    __shared__ int s_pos[SNMS_T / 64];
    __shared__ int s_scan[SNMS_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < n; i += SNMS_T) inds[i] = i;
    __syncthreads();
    int N = n;
    for (int i = 0; i < N; ++i) {
        // ---- arg-max over [i, N): first position holding the maximum score
        float bv = -INFINITY; int bp = 0x7fffffff;
        for (int p = i + tid; p < N; p += SNMS_T) { float s = boxes[p * 5 + 4]; if (s > bv) { bv = s; bp = p; } }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            float ov = __shfl_down(bv, d, 64); int op = __shfl_down(bp, d, 64);
            if (ov > bv || (ov == bv && op < bp)) { bv = ov; bp = op; }
        }
        if (lane == 0) { s_val[wave] = bv; s_pos[wave] = bp; }
        __syncthreads();
        if (tid == 0) {
            float v = s_val[0]; int p = s_pos[0];
            for (int w = 1; w < SNMS_T / 64; ++w) if (s_val[w] > v || (s_val[w] == v && s_pos[w] < p)) { v = s_val[w]; p = s_pos[w]; }
            // reference starts from maxpos = i and moves only on a strictly larger score
            if (!(boxes[i * 5 + 4] < v)) p = i;
            if (p != i) {
                for (int k = 0; k < 5; ++k) { float t = boxes[i * 5 + k]; boxes[i * 5 + k] = boxes[p * 5 + k]; boxes[p * 5 + k] = t; }
                int64_t ti = inds[i]; inds[i] = inds[p]; inds[p] = ti;
            }
        }
        __syncthreads();
        const float tx1 = boxes[i * 5 + 0], ty1 = boxes[i * 5 + 1], tx2 = boxes[i * 5 + 2], ty2 = boxes[i * 5 + 3];
        // ---- re-score (i, N) and flag removals
        for (int p = i + 1 + tid; p < N; p += SNMS_T) {
            const float x1 = boxes[p * 5 + 0], y1 = boxes[p * 5 + 1], x2 = boxes[p * 5 + 2], y2 = boxes[p * 5 + 3];
            uint8_t rem = 0;
            float ns = boxes[p * 5 + 4];
            if (snms_rescore(tx1, ty1, tx2, ty2, x1, y1, x2, y2, sigma, Nt, method, &ns)) { boxes[p * 5 + 4] = ns; rem = ns < threshold; }
            flag[p] = rem;
        }
        __syncthreads();
        // ---- compaction: survivors keep their slot if < N'; holes below N' take survivors from the end
        const int len = N - (i + 1);
        if (len > 0) {
            int nrem_total = 0;
            // count removed
            int local = 0;
            for (int p = i + 1 + tid; p < N; p += SNMS_T) local += flag[p];
            (void)block_excl_scan(local, s_scan, &nrem_total);
            if (nrem_total > 0) {
                const int Nn = N - nrem_total;
                // holes: removed positions < Nn, ranked ascending; movers: surviving positions >= Nn, ranked descending.
                // Both sets have equal size (<= nrem_total). Chunked ranks keep position order across chunks.
                int hole_base = 0, mover_base = 0;
                const int chunks = (len + SNMS_T - 1) / SNMS_T;
                for (int c = 0; c < chunks; ++c) {
                    const int p = i + 1 + c * SNMS_T + tid;            // ascending walk for holes
                    const int ish = (p < Nn) && flag[p];
                    int tot; const int r = block_excl_scan(ish, s_scan, &tot);
                    if (ish) tmp_ind[hole_base + r] = p;                // hole list (position)
                    hole_base += tot;
                }
                for (int c = 0; c < chunks; ++c) {
                    const int p = N - 1 - (c * SNMS_T + tid);          // descending walk for movers
                    const int ism = (p >= Nn) && (p > i) && !flag[p];
                    int tot; const int r = block_excl_scan(ism, s_scan, &tot);
                    if (ism) {
                        for (int k = 0; k < 5; ++k) tmp_box[(mover_base + r) * 5 + k] = boxes[p * 5 + k];
                        tmp_box[(size_t)n * 5 + mover_base + r] = __builtin_bit_cast(float, (int)p);
                    }
                    mover_base += tot;
                }
                __syncthreads();
                for (int q = tid; q < hole_base; q += SNMS_T) {
                    const int dst = (int)tmp_ind[q];
                    const int src = __builtin_bit_cast(int, tmp_box[(size_t)n * 5 + q]);
                    for (int k = 0; k < 5; ++k) boxes[dst * 5 + k] = tmp_box[q * 5 + k];
                    flag[dst] = 2;  // marks "index must be taken from src"
                    tmp_ind[n + q] = inds[src];
                }
                __syncthreads();
                for (int q = tid; q < hole_base; q += SNMS_T) inds[(int)tmp_ind[q]] = tmp_ind[n + q];
                N = Nn;
            }
        }
        __syncthreads();
    }
    if (tid == 0) *n_out = N;
}

extern "C" size_t upsnet_soft_nms_batched_workspace_bytes(int P, int nmax)
{
    if (P <= 0 || nmax <= SNMS_LDS_MAX) return 256;   // the LDS form needs no scratch
    const size_t per = (size_t)nmax * 6 * sizeof(float) + (size_t)nmax * 2 * sizeof(int64_t) + (size_t)nmax;
    return align256((size_t)P * per) + 3 * 256;
}

extern "C" int upsnet_soft_nms_batched(void *stream, float *boxes, int64_t *inds, const int *counts, int P, int nmax, float sigma,
                                       float Nt, float threshold, int method, int *n_out, void *workspace)
{
    UPS_REQUIRE(boxes && inds && n_out, "soft_nms_batched: null pointer");
    UPS_REQUIRE(P >= 0 && nmax >= 0 && nmax < (1 << 24), "soft_nms_batched: bad sizes P=%d nmax=%d", P, nmax);
    UPS_REQUIRE(method >= 0 && method <= 2, "soft_nms_batched: method must be 0 (hard), 1 (linear) or 2 (gaussian)");
    if (P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (nmax == 0) { return ups_zero_async(n_out, (size_t)P * sizeof(int), st); }
    if (nmax <= SNMS_LDS_MAX) {
        const int T = nmax <= 64 * SNMS_KMAX ? 64 : 256;
        const int cap = (nmax + 3) & ~3;
        const size_t smem = snms_lds_bytes(cap);
        if (T == 64) {
            hipLaunchKernelGGL(soft_nms_lds_kernel<64>, dim3(P), dim3(64), smem, st, boxes, inds, counts, nmax, cap, sigma, Nt,
                               threshold, method, n_out);
        } else {
            static std::atomic<unsigned long long> attr_dev{0};
            UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&soft_nms_lds_kernel<256>),
                                                                            hipFuncAttributeMaxDynamicSharedMemorySize, SNMS_LDS_MAX * 28)));
            hipLaunchKernelGGL(soft_nms_lds_kernel<256>, dim3(P), dim3(256), smem, st, boxes, inds, counts, nmax, cap, sigma, Nt,
                               threshold, method, n_out);
        }
        UPS_CHECK_LAUNCH("soft_nms_lds_kernel");
        return 0;
    }
    UPS_REQUIRE(workspace, "soft_nms_batched: workspace required for nmax > %d", SNMS_LDS_MAX);
    unsigned char *b = (unsigned char *)workspace;
    float *tmp_box = (float *)b; b += align256((size_t)P * nmax * 6 * sizeof(float));
    int64_t *tmp_ind = (int64_t *)b; b += align256((size_t)P * nmax * 2 * sizeof(int64_t));
    uint8_t *flag = b;
    hipLaunchKernelGGL(soft_nms_kernel, dim3(P), dim3(SNMS_T), 0, st, boxes, inds, counts, nmax, sigma, Nt, threshold, method,
                       n_out, tmp_box, tmp_ind, flag);
    UPS_CHECK_LAUNCH("soft_nms_kernel");
    return 0;
}

// single problem (the r01 entry point): P = 1, all n rows valid
extern "C" size_t upsnet_soft_nms_workspace_bytes(int n) { return upsnet_soft_nms_batched_workspace_bytes(1, n); }

extern "C" int upsnet_soft_nms(void *stream, float *boxes, int64_t *inds, int n, float sigma, float Nt, float threshold, int method,
                               int *n_out, void *workspace)
{
    return upsnet_soft_nms_batched(stream, boxes, inds, nullptr, 1, n, sigma, Nt, threshold, method, n_out, workspace);
}
