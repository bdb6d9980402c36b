// soft_nms_trips.h -- the sequential trips of cpu_soft_nms (cpu_nms.pyx:91-196) on a problem whose state lives in LDS.
//
// One body for both users, so that they cannot drift: soft_nms_lds_kernel (nms.hip, the stand-alone batched entry point) and
// mroi_soft_kernel (detect.hip, the soft detection selection). The caller fills the structure-of-arrays state
// (x1 / y1 / x2 / y2 / score / index, positions 0..n-1), synchronises, and calls snms_lds_trips<T> with all T threads of the workgroup;
// on return (after a barrier) positions 0..N'-1 hold cpu_soft_nms's result and the value returned is N'. `ind` is only permuted with
// the boxes: whatever the caller put there (the position, or a source row) comes back in the reference's order.
//
// A trip is: arg-max over [i, N) (first position of the maximum, :113-118), swap (:120-135), re-score of (i, N) (:147-180) and the
// reference's "swap with last" compaction (:184-193) restated as: k-th hole (ascending) <- k-th survivor from the end (descending),
// with N' = N - #removed.
//
// Arithmetic: Cython widens the literal in `x2 - x1 + 1` to the C double 1.0, so `area` and `ua` are evaluated in double from
// fp32 differences and rounded once (see oracle/c/upsnet_oracle.c orc_soft_nms; pinned against the compiled reference).
#pragma once
#include "common.h"

#define SNMS_KMAX 16     // chunks of T positions per trip: T * SNMS_KMAX >= n
#define SNMS_LDS_MAX 4096

__device__ static inline bool snms_rescore(const float tx1, const float ty1, const float tx2, const float ty2, const float bx1,
                                           const float by1, const float bx2, const float by2, const float sigma, const float Nt,
                                           const int method, float *score)
{
    const float area = (float)(((double)(bx2 - bx1) + 1.0) * ((double)(by2 - by1) + 1.0));
    const float iw = (float)((double)(fminf(tx2, bx2) - fmaxf(tx1, bx1)) + 1.0);
    if (!(iw > 0)) return false;
    const float ih = (float)((double)(fminf(ty2, by2) - fmaxf(ty1, by1)) + 1.0);
    if (!(ih > 0)) return false;
    const float ua = (float)(((((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0)) + (double)area) - (double)(iw * ih));
    const float ov = iw * ih / ua;
    float weight;
    if (method == 1) weight = ov > Nt ? (float)(1.0 - (double)ov) : 1.0f;
    else if (method == 2) weight = (float)exp((double)(-(ov * ov) / sigma));
    else weight = ov > Nt ? 0.0f : 1.0f;
    *score = weight * *score;
    return true;
}

// dynamic LDS bytes of a problem of up to `cap` boxes (cap a multiple of 4): six 4-byte arrays and the two position lists
static inline size_t snms_lds_bytes(int cap) { return (size_t)cap * (5 * sizeof(float) + sizeof(int) + 2 * sizeof(unsigned short)); }

// the cross-wave scratch of the trips (static LDS of the calling kernel)
template <int T>
struct SnmsScratch {
    int tab[3][SNMS_KMAX][T / 64];
    float val[T / 64];
    int pos[T / 64];
};

// the state arrays carved from the kernel's dynamic LDS (cap boxes each)
struct SnmsState {
    float *x1, *y1, *x2, *y2, *sc;
    int *ind;
    unsigned short *hole, *mover;
};

__device__ static inline SnmsState snms_carve(unsigned char *smem, const int cap)
{
    SnmsState s;
    s.x1 = reinterpret_cast<float *>(smem); s.y1 = s.x1 + cap; s.x2 = s.y1 + cap; s.y2 = s.x2 + cap; s.sc = s.y2 + cap;
    s.ind = reinterpret_cast<int *>(s.sc + cap);
    s.hole = reinterpret_cast<unsigned short *>(s.ind + cap); s.mover = s.hole + cap;
    return s;
}

template <int T>
__device__ static inline int snms_lds_trips(const SnmsState &st, SnmsScratch<T> &ss, const int n, const float sigma, const float Nt,
                                            const float threshold, const int method)
{
    constexpr int W = T / 64;
    typedef unsigned long long u64_;
    float *x1 = st.x1, *y1 = st.y1, *x2 = st.x2, *y2 = st.y2, *sc = st.sc;
    int *ind = st.ind;
    unsigned short *hole = st.hole, *mover = st.mover;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const u64_ lt = (1ULL << lane) - 1ULL;
    int N = n;
    for (int i = 0; i < N; ++i) {
        // ---- arg-max over [i, N): first position holding the maximum score (a thread walks ascending positions, `>` keeps the first)
        float bv = -INFINITY; int bp = 0x7fffffff;
        for (int q = i + tid; q < N; q += T) { const float v = sc[q]; if (v > bv) { bv = v; bp = q; } }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const float ov = __shfl_xor(bv, d, 64); const int op = __shfl_xor(bp, d, 64);
            if (ov > bv || (ov == bv && op < bp)) { bv = ov; bp = op; }
        }
        if (W > 1) {
            if (lane == 0) { ss.val[wave] = bv; ss.pos[wave] = bp; }
            __syncthreads();
            bv = ss.val[0]; bp = ss.pos[0];
#pragma unroll
            for (int w = 1; w < W; ++w) { const float ov = ss.val[w]; const int op = ss.pos[w]; if (ov > bv || (ov == bv && op < bp)) { bv = ov; bp = op; } }
        }
        if (!(sc[i] < bv)) bp = i;   // the reference starts from maxpos = i and moves only on a strictly larger score
        __syncthreads();
        if (tid == 0 && bp != i) {
            float t;
            t = x1[i]; x1[i] = x1[bp]; x1[bp] = t;  t = y1[i]; y1[i] = y1[bp]; y1[bp] = t;
            t = x2[i]; x2[i] = x2[bp]; x2[bp] = t;  t = y2[i]; y2[i] = y2[bp]; y2[bp] = t;
            t = sc[i]; sc[i] = sc[bp]; sc[bp] = t;
            const int ti = ind[i]; ind[i] = ind[bp]; ind[bp] = ti;
        }
        __syncthreads();
        const float tx1 = x1[i], ty1 = y1[i], tx2 = x2[i], ty2 = y2[i];
        // ---- re-score (i, N); chunk k covers positions i+1+k*T .. +T-1, bit k of `rem` = "my position of chunk k falls below threshold"
        const int len = N - (i + 1);
        const int K = (len + T - 1) / T;
        unsigned rem = 0;
        int my_removed = 0;
        for (int k = 0; k < K; ++k) {
            const int q = i + 1 + k * T + tid;
            bool r = false;
            if (q < N) {
                float ns = sc[q];
                if (snms_rescore(tx1, ty1, tx2, ty2, x1[q], y1[q], x2[q], y2[q], sigma, Nt, method, &ns)) { sc[q] = ns; r = ns < threshold; }
            }
            const u64_ m = __ballot(r);
            if (r) rem |= 1u << k;
            if (W > 1) { if (lane == 0) ss.tab[0][k][wave] = __builtin_popcountll(m); }
            else my_removed += __builtin_popcountll(m);
        }
        int R = my_removed;
        if (W > 1) {
            __syncthreads();
            R = 0;
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int w = 0; w < W; ++w) R += ss.tab[0][k][w];
        }
        if (R == 0) { if (W > 1) __syncthreads(); continue; }
        const int Nn = N - R;
        // ---- holes (removed, position < Nn) ranked ascending; movers (survivors at positions >= Nn) ranked ascending, used descending
        int hole_base = 0, mover_base = 0;
        if (W > 1) {
            for (int k = 0; k < K; ++k) {
                const int q = i + 1 + k * T + tid;
                const bool r = (rem >> k) & 1u;
                const u64_ mh = __ballot(q < Nn && r), mm = __ballot(q >= Nn && q < N && !r);
                if (lane == 0) { ss.tab[1][k][wave] = __builtin_popcountll(mh); ss.tab[2][k][wave] = __builtin_popcountll(mm); }
            }
            __syncthreads();
        }
        int n_holes = 0, n_movers = 0;
        if (W > 1) {
            for (int k = 0; k < K; ++k)
#pragma unroll
                for (int w = 0; w < W; ++w) { n_holes += ss.tab[1][k][w]; n_movers += ss.tab[2][k][w]; }
        } else {
            for (int k = 0; k < K; ++k) {
                const int q = i + 1 + k * T + tid;
                const bool r = (rem >> k) & 1u;
                n_holes += __builtin_popcountll(__ballot(q < Nn && r));
                n_movers += __builtin_popcountll(__ballot(q >= Nn && q < N && !r));
            }
        }
        for (int k = 0; k < K; ++k) {
            const int q = i + 1 + k * T + tid;
            const bool r = (rem >> k) & 1u;
            const bool ish = q < Nn && r, ism = q >= Nn && q < N && !r;
            const u64_ mh = __ballot(ish), mm = __ballot(ism);
            int hb = hole_base, mb = mover_base;
            if (W > 1) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    if (w < wave) { hb += ss.tab[1][k][w]; mb += ss.tab[2][k][w]; }
                    hole_base += ss.tab[1][k][w]; mover_base += ss.tab[2][k][w];
                }
            } else {
                hole_base += __builtin_popcountll(mh); mover_base += __builtin_popcountll(mm);
            }
            if (ish) hole[hb + __builtin_popcountll(mh & lt)] = (unsigned short)q;
            if (ism) mover[n_movers - 1 - (mb + __builtin_popcountll(mm & lt))] = (unsigned short)q;
        }
        __syncthreads();
        for (int j = tid; j < n_holes; j += T) {   // n_holes == n_movers
            const int dst = hole[j], src = mover[j];
            x1[dst] = x1[src]; y1[dst] = y1[src]; x2[dst] = x2[src]; y2[dst] = y2[src]; sc[dst] = sc[src]; ind[dst] = ind[src];
        }
        __syncthreads();
        N = Nn;
    }
    __syncthreads();   // (the last trip may have left through `continue`: the caller reads other threads' positions next)
    return N;
}
