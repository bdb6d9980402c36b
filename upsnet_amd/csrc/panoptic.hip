// panoptic.hip -- the parameter-free panoptic head on the device (gfx950).
//
// Reference (all host/Python): MaskRemoval (upsnet/operators/modules/mask_removal.py:29-93: cv2.resize
// per instance on the CPU, per-instance H2D copies, an [m,H,W] fp32 memset), SegTerm
// (upsnet/operators/modules/unary_logits.py:78-105: Python loop + [k,H,W] memset) and the fusion in
// upsnet/models/resnet_upsnet.py:234-243 (max / cat / argmax over (12+2k) full-resolution planes).
//
// Here:
//  * mask_removal_kernel  : one workgroup per thing class walks that class's instances in global
//    score order; the 28x28 logits are resampled on the fly (INTER_LINEAR restated), mask_sum and the
//    overlap with the class occupancy plane are integer workgroup reductions -> decisions bit-exact.
//  * panoptic_fuse_kernel : ONE pass over fcn_output produces the panoptic (and semantic) label map;
//    instance logits (SegTerm crop + pasted mask logit) are evaluated per pixel from the box list,
//    nothing of size [k,H,W] is ever materialised: ~(S*4 + 16) bytes per pixel instead of ~(12+2k)*24.
//  * mask_paste / seg_term / panoptic_argmax: materialising variants that keep the reference's
//    module-level API (MaskRemoval returns mask_energy, SegTerm returns seg_inst_energy).
#include "common.h"
#include "sort.h"
#include "upsnet_hip.h"

#define PAN_T 1024
static inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
#define PAN_MAXDIM 4096   // max box side handled by the removal kernel's coefficient tables
#define PAN_MAXINST 1024  // max instances entering mask removal
#define PAN_MAXMS 32      // max mask side (28 in every config)

#include "resize.h"

struct PanBox {  // MaskRemoval geometry of one instance (mask_removal.py:60-77)
    int bx0, by0, w, h, x_0, x_1, y_0, y_1;
};
__device__ static inline PanBox pan_box(const float *__restrict__ r4, int H, int W)
{
    PanBox b;
    const int x1 = (int)r4[0], y1 = (int)r4[1], x2 = (int)r4[2], y2 = (int)r4[3];  // astype(int32): truncation
    b.bx0 = x1; b.by0 = y1;
    b.w = max(x2 - x1 + 1, 1); b.h = max(y2 - y1 + 1, 1);
    b.x_0 = max(x1, 0); b.x_1 = min(x2 + 1, W);
    b.y_0 = max(y1, 0); b.y_1 = min(y2 + 1, H);
    // python slicing of the h x w mask clamps the stop: local coords stay < (h, w)
    b.x_1 = min(b.x_1, x1 + b.w); b.y_1 = min(b.y_1, y1 + b.h);
    return b;
}

__device__ static inline long pan_block_sum(long v, long *sh)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned lo = __shfl_down((unsigned)v, d, 64), hi = __shfl_down((unsigned)((unsigned long long)v >> 32), d, 64);
        v += (long)(((unsigned long long)hi << 32) | lo);
    }
    __syncthreads();
    if (lane == 0) sh[wave] = v;
    __syncthreads();
    long t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w];
    return t;
}

// Mask removal in two phases.
//  A (mask_bits_kernel, fully parallel over instances x rows x 64-pixel words): resample each instance's 28x28
//    logits into its box, threshold (> 0) and pack the result as a bitmap aligned to image columns
//    (bits[(inst*H + y)*WW + x/64]); mask_sum[inst] = popcount total.
//  B (mask_removal_kernel, one workgroup per thing class): walk that class's instances in global score order;
//    overlap = popcount(bits & occupancy_bits[class]) over the box, decide with the reference's integer/fp64 rule
//    (mask_removal.py:82), OR the kept bitmap into the class occupancy. The per-instance critical path is a few
//    microseconds of 64-bit AND/popcount instead of a full resample of the box.
__global__ void __launch_bounds__(256)
mask_bits_kernel(const float *__restrict__ rois, const float *__restrict__ logits, const int m_cap, const int *__restrict__ m_dev,
                 const int ms, const int H, const int W, const int WW, unsigned long long *__restrict__ bits, int *__restrict__ mask_sum)
{
    __shared__ float s_logit[PAN_MAXMS * PAN_MAXMS];
    if ((int)blockIdx.x >= (m_dev ? min(m_cap, *m_dev) : m_cap)) return;   // fixed-capacity launch, device-side count
    const int inst = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int q = tid; q < ms * ms; q += blockDim.x) s_logit[q] = logits[(long)inst * ms * ms + q];
    __syncthreads();
    const PanBox b = pan_box(rois + (long)inst * 4, H, W);
    const int rx = b.x_1 - b.x_0, ry = b.y_1 - b.y_0;
    if (rx <= 0 || ry <= 0) return;
    const int wc0 = b.x_0 >> 6, nw = ((b.x_1 - 1) >> 6) - wc0 + 1;
    const long items = (long)ry * nw;
    int local = 0;
    for (long it = (long)blockIdx.y * 4 + wave; it < items; it += (long)gridDim.y * 4) {
        const int yy = (int)(it / nw), wc = wc0 + (int)(it % nw);
        const int y = b.y_0 + yy, x = wc * 64 + lane;
        bool on = false;
        if (x >= b.x_0 && x < b.x_1) on = pan_resize_at(s_logit, ms, b.w, b.h, x - b.bx0, y - b.by0) > 0;
        const unsigned long long word = __ballot(on);
        if (lane == 0) { bits[((long)inst * H + y) * WW + wc] = word; local += __builtin_popcountll(word); }
    }
    if (lane == 0 && local) atomicAdd(&mask_sum[inst], local);
}

// grid = num_thing_classes, block = MR_T (4 waves). r08 rewrite.
// The reference walks the instances in score order and keeps a per-class occupancy plane (mask_removal.py:60-89): an instance is
// kept unless more than `fraction` of its mask is already occupied by KEPT earlier instances of its class. r01-r07 restated that
// literally -- one instance after the other, read-modify-write of a global occupancy bit-plane, a workgroup reduction and two
// barriers per instance: 5-9 us per instance, 89-127 us per image, all of it latency. But the decision of instance i depends only
// on the decisions of the earlier same-class instances whose BOXES intersect its box (usually none or one or two), and the
// occupancy inside box i is just the OR of those instances' bitmaps, which are static (mask_bits_kernel). So:
//   * rounds instead of a walk: in every round each undecided instance whose intersecting predecessors are all decided is resolved
//     -- independent instances in parallel, one wavefront each, no workgroup reduction;
//   * no occupancy plane: overlap_i = popcount(bits_i & OR_{kept j < i, box_j meets box_i} bits_j) over box i, read-only data;
//   * the number of rounds is the longest chain of intersecting boxes (2-4 in practice), not the number of instances.
// Decisions are the reference's, bit for bit: same integer overlap, same fp64 ratio test.
#define MR_T 256
#define MR_MAXCAND 64
struct MrBox { int x0, x1, y0, y1; };   // clipped pixel box [x0, x1) x [y0, y1); empty if x1 <= x0 or y1 <= y0

__global__ void __launch_bounds__(MR_T)
mask_removal_kernel(const float *__restrict__ rois, const float *__restrict__ prob, const int64_t *__restrict__ cls_idx,
                    const int m_cap, const int *__restrict__ m_dev, const int H, const int W, const int WW,
                    const double fraction_threshold, const unsigned long long *__restrict__ bits, const int *__restrict__ mask_sum,
                    unsigned long long *__restrict__ occbits, int *__restrict__ sorted_idx, uint8_t *__restrict__ kept_flag)
{
    (void)occbits;
    const int m = m_dev ? min(m_cap, *m_dev) : m_cap;
    __shared__ ups_u64 s_keys[PAN_MAXINST];
    __shared__ int s_pos[PAN_MAXINST];          // this class's instances in score order: position in the global score order ...
    __shared__ int s_inst[PAN_MAXINST];         // ... and instance index
    __shared__ MrBox s_box[PAN_MAXINST];
    __shared__ int s_sum[PAN_MAXINST];
    __shared__ unsigned char s_state[PAN_MAXINST];   // 0 undecided, 1 kept, 2 dropped
    __shared__ unsigned char s_ready[PAN_MAXINST];
    __shared__ int s_cand[MR_T / 64][MR_MAXCAND];
    __shared__ int s_nmy, s_left;
    const int tid = threadIdx.x, my_cls = blockIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = ups_next_pow2(m < 64 ? 64 : m);
    for (int i = tid; i < M; i += MR_T) s_keys[i] = i < m ? ups_make_key(prob[i], (unsigned)i, 0) : 0ULL;
    if (M <= 256) ups_block_rank_sort_desc(s_keys, m, M);   // (unique, non-zero keys; see sort.h for the size rule)
    else ups_block_sort_desc(s_keys, M);
    // ---- ordered compaction of this class's instances (one wave, 64 score positions per trip)
    for (int t = tid; t < m; t += MR_T) {
        const int idx = (int)ups_key_index(s_keys[t], 0);
        if (my_cls == 0) sorted_idx[t] = idx;
        s_pos[t] = ((int)cls_idx[idx] - 1 == my_cls) ? idx : -1;       // (class flag until the compaction below)
    }
    __syncthreads();
    if (wave == 0) {
        int base = 0;
        for (int t0 = 0; t0 < m; t0 += 64) {
            const int t = t0 + lane;
            const int idx = t < m ? s_pos[t] : -1;
            const unsigned long long bal = __ballot(idx >= 0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // (the reads of s_pos above stay above the writes below)
            __builtin_amdgcn_wave_barrier();
            if (idx >= 0) {
                const int pos = base + __builtin_popcountll(bal & ((1ULL << lane) - 1ULL));   // pos <= t: that slot has been read
                const PanBox b = pan_box(rois + (long)idx * 4, H, W);
                MrBox mb;
                mb.x0 = b.x_0; mb.x1 = b.x_1; mb.y0 = b.y_0; mb.y1 = b.y_1;
                const int sum = mask_sum[idx];
                const bool live = mb.x1 > mb.x0 && mb.y1 > mb.y0 && sum > 0;
                s_pos[pos] = t; s_inst[pos] = idx; s_box[pos] = mb; s_sum[pos] = sum;
                s_state[pos] = live ? 0 : 2;
                if (!live) kept_flag[t] = 0;
            }
            base += __builtin_popcountll(bal);
        }
        if (lane == 0) s_nmy = base;
    }
    __syncthreads();
    const int n_my = s_nmy;
#define MR_MEET(A, B) ((A).x0 < (B).x1 && (B).x0 < (A).x1 && (A).y0 < (B).y1 && (B).y0 < (A).y1)
    for (;;) {
        // ---- which undecided instances have all their intersecting predecessors decided?
        if (tid == 0) s_left = 0;
        __syncthreads();
        int mine_left = 0;
        for (int i = tid; i < n_my; i += MR_T) {
            bool ready = false;
            if (s_state[i] == 0) {
                ready = true;
                const MrBox bi = s_box[i];
                for (int j = 0; j < i; ++j)
                    if (s_state[j] == 0 && MR_MEET(bi, s_box[j])) { ready = false; break; }
                ++mine_left;
            }
            s_ready[i] = ready ? 1 : 0;
        }
        if (mine_left) atomicAdd(&s_left, mine_left);
        __syncthreads();
        if (s_left == 0) break;
        // ---- resolve the ready ones, one wavefront per instance (the r-th ready instance goes to wave r mod 4)
        int r = 0;
        for (int i = 0; i < n_my; ++i) {
            if (!s_ready[i]) continue;
            if ((r++ & (MR_T / 64 - 1)) != wave) continue;
            const MrBox bi = s_box[i];
            // kept predecessors whose box meets this one (lane-parallel scan, ballot compaction into the wave's list)
            int ncand = 0;
            for (int j0 = 0; j0 < i; j0 += 64) {
                const int j = j0 + lane;
                const bool c = j < i && s_state[j] == 1 && MR_MEET(bi, s_box[j]);
                const unsigned long long bal = __ballot(c);
                if (c) { const int at = ncand + __builtin_popcountll(bal & ((1ULL << lane) - 1ULL)); if (at < MR_MAXCAND) s_cand[wave][at] = j; }
                ncand += __builtin_popcountll(bal);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const bool listed = ncand <= MR_MAXCAND;     // (more than 64 overlapping kept predecessors: scan all of them instead)
            const int wc0 = bi.x0 >> 6, nw = ((bi.x1 - 1) >> 6) - wc0 + 1;
            const long items = (long)(bi.y1 - bi.y0) * nw;
            const unsigned long long *__restrict__ bsrc = bits + (long)s_inst[i] * H * WW;
            long ov = 0;
            if (ncand > 0) {
                for (long it = lane; it < items; it += 64) {
                    const int y = bi.y0 + (int)(it / nw), wc = wc0 + (int)(it % nw);
                    const long off = (long)y * WW + wc;
                    const unsigned long long w = bsrc[off];
                    unsigned long long occ = 0;
                    const int nscan = listed ? ncand : i;
                    for (int c = 0; c < nscan; ++c) {
                        const int j = listed ? s_cand[wave][c] : c;
                        if (!listed && !(s_state[j] == 1)) continue;
                        const MrBox bj = s_box[j];
                        // instance j's bitmap holds defined words only inside its own box rows / words
                        if (y >= bj.y0 && y < bj.y1 && wc >= (bj.x0 >> 6) && wc <= ((bj.x1 - 1) >> 6))
                            occ |= bits[(long)s_inst[j] * H * WW + off];
                    }
                    ov += __builtin_popcountll(w & occ);
                }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) {
                    const unsigned lo = __shfl_xor((unsigned)ov, d, 64), hi = __shfl_xor((unsigned)((unsigned long long)ov >> 32), d, 64);
                    ov += (long)(((unsigned long long)hi << 32) | lo);
                }
            }
            const bool keep = !((double)ov / (double)s_sum[i] > fraction_threshold);  // mask_removal.py:82
            if (lane == 0) { s_state[i] = keep ? 1 : 2; kept_flag[s_pos[i]] = keep ? 1 : 0; }
        }
        __syncthreads();
    }
#undef MR_MEET
}

__global__ void __launch_bounds__(256)
mask_removal_finalize_kernel(const int64_t *__restrict__ cls_idx, const int m_cap, const int *__restrict__ m_dev,
                             const int *__restrict__ sorted_idx, const uint8_t *__restrict__ kept_flag, int64_t *__restrict__ keep_inds,
                             int *__restrict__ num_keep, int *__restrict__ real_keep)
{
    __shared__ int k_sh;
    if (threadIdx.x == 0) {
        const int m = m_dev ? min(m_cap, *m_dev) : m_cap;
        int k = 0;
        const bool dummy = (m == 1 && cls_idx[0] == 0);  // mask_removal.py:55-57
        if (!dummy)
            for (int si = 0; si < m; ++si) if (kept_flag[si]) keep_inds[k++] = sorted_idx[si];
        if (k == 0) { keep_inds[0] = 0; *num_keep = 1; *real_keep = 0; k = 1; }  // :90-92
        else { *num_keep = k; *real_keep = 1; }
        k_sh = k;
    }
    __syncthreads();
    // rows past the count are defined (0), so the caller need not clear the buffer
    for (int i = k_sh + (int)threadIdx.x; i < m_cap; i += (int)blockDim.x) keep_inds[i] = 0;
}

// Tail of the fixed-capacity forward: the kept detections' classes / scores (rows past num_keep: as if keep were 0, like the
// index_select of a zero-filled index buffer) and the four device counters the host reads after the replay, in one launch
// (instead of clamp + 2 x index_select + 2 x cat).
__global__ void __launch_bounds__(256)
pan_tail_pack_kernel(const int64_t *__restrict__ keep, const int *__restrict__ num_keep, const int K, const int64_t *__restrict__ cls,
                     const float *__restrict__ scores, const int *__restrict__ det_num, const int *__restrict__ pan_num,
                     const int *__restrict__ extra_num, int64_t *__restrict__ kept_cls, float *__restrict__ kept_scores,
                     int *__restrict__ counters)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int nk = *num_keep;
    if (i < K) {
        long kk = i < nk ? (long)keep[i] : 0;
        kk = kk < 0 ? 0 : (kk > K - 1 ? K - 1 : kk);
        kept_cls[i] = cls[kk];
        kept_scores[i] = scores[kk];
    }
    if (i == 0) { counters[0] = *det_num; counters[1] = *pan_num; counters[2] = *extra_num; counters[3] = nk; }
}

extern "C" int upsnet_panoptic_tail_pack(void *stream, const int64_t *keep, const int *num_keep, int K, const int64_t *cls,
                                         const float *scores, const int *det_num, const int *pan_num, const int *extra_num,
                                         int64_t *kept_cls, float *kept_scores, int *counters)
{
    UPS_REQUIRE(keep && num_keep && cls && scores && det_num && pan_num && extra_num && kept_cls && kept_scores && counters && K >= 1,
                "panoptic_tail_pack: null pointer / K < 1");
    hipLaunchKernelGGL(pan_tail_pack_kernel, dim3(ups_divup(K, 256)), dim3(256), 0, (hipStream_t)stream, keep, num_keep, K, cls, scores,
                       det_num, pan_num, extra_num, kept_cls, kept_scores, counters);
    UPS_CHECK_LAUNCH("pan_tail_pack_kernel");
    return 0;
}

struct MrPlan { size_t occ, bits, sums, sorted, kept, total; int WW; };
static MrPlan mr_plan(int m, int ncls, int H, int W)
{
    MrPlan p;
    if (m < 1) m = 1;
    if (ncls < 1) ncls = 1;
    p.WW = (int)(((long)W + 63) / 64);
    size_t o = 0;
    p.occ = o; o += al256((size_t)ncls * H * p.WW * 8);
    p.bits = o; o += al256((size_t)m * H * p.WW * 8);
    p.sums = o; o += al256((size_t)m * 4);
    p.kept = o; o += al256((size_t)m);          // (directly behind `sums`: one zero-fill launch covers both)
    p.sorted = o; o += al256((size_t)m * 4);
    p.total = o + 256;
    return p;
}

extern "C" size_t upsnet_mask_removal_workspace_bytes(int m, int ncls, int H, int W) { return mr_plan(m, ncls, H, W).total; }

extern "C" int upsnet_mask_removal(void *stream, const float *mask_rois, const float *cls_prob, const float *mask_logit,
                                   const int64_t *cls_idx, int m, const int *m_dev, int mask_size, int ncls, int H, int W,
                                   double fraction_threshold, int64_t *keep_inds, int *num_keep, int *real_keep,
                                   void *workspace)
{
    UPS_REQUIRE(mask_rois && cls_prob && mask_logit && cls_idx && keep_inds && num_keep && real_keep && workspace,
                "mask_removal: null pointer");
    UPS_REQUIRE(m >= 1 && m <= PAN_MAXINST, "mask_removal: m must be 1..%d (got %d)", PAN_MAXINST, m);
    UPS_REQUIRE(mask_size >= 2 && mask_size <= PAN_MAXMS, "mask_removal: mask_size must be 2..%d", PAN_MAXMS);
    UPS_REQUIRE(ncls >= 1 && H >= 1 && W >= 1, "mask_removal: bad class count / image size");
    const MrPlan pl = mr_plan(m, ncls, H, W);
    unsigned char *ws = (unsigned char *)workspace;
    unsigned long long *occ = (unsigned long long *)(ws + pl.occ), *bits = (unsigned long long *)(ws + pl.bits);
    int *sums = (int *)(ws + pl.sums), *sorted_idx = (int *)(ws + pl.sorted);
    uint8_t *kept = ws + pl.kept;
    hipStream_t st = (hipStream_t)stream;
    if (ups_zero_async(sums, (pl.kept - pl.sums) + (((size_t)m + 3) & ~(size_t)3), st)) return 1;   // sums + kept (adjacent, 256-byte padded slots)
    hipLaunchKernelGGL(mask_bits_kernel, dim3(m, 32), dim3(256), 0, st, mask_rois, mask_logit, m, m_dev, mask_size, H, W, pl.WW, bits, sums);
    UPS_CHECK_LAUNCH("mask_bits_kernel");
    hipLaunchKernelGGL(mask_removal_kernel, dim3(ncls), dim3(MR_T), 0, st, mask_rois, cls_prob, cls_idx, m, m_dev, H, W, pl.WW,
                       fraction_threshold, bits, sums, occ, sorted_idx, kept);
    UPS_CHECK_LAUNCH("mask_removal_kernel");
    hipLaunchKernelGGL(mask_removal_finalize_kernel, dim3(1), dim3(64), 0, st, cls_idx, m, m_dev, sorted_idx, kept, keep_inds, num_keep,
                       real_keep);
    UPS_CHECK_LAUNCH("mask_removal_finalize_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// materialisers (module-level API parity)
__global__ void __launch_bounds__(256)
mask_paste_kernel(const float *__restrict__ rois, const float *__restrict__ logits, const int64_t *__restrict__ keep_inds,
                  const int *__restrict__ num_keep, const int *__restrict__ real_keep, const int ms, const int H, const int W,
                  float *__restrict__ energy)
{
    const int j = blockIdx.y;
    const long hw = (long)H * W;
    const bool live = j < *num_keep && *real_keep;
    PanBox b = {};
    const float *src = logits;
    if (live) { const long i = keep_inds[j]; b = pan_box(rois + i * 4, H, W); src = logits + i * ms * ms; }
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long)blockDim.x * gridDim.x) {
        const int y = (int)(p / W), x = (int)(p % W);
        float v = 0.f;
        if (live && y >= b.y_0 && y < b.y_1 && x >= b.x_0 && x < b.x_1) v = pan_resize_at(src, ms, b.w, b.h, x - b.bx0, y - b.by0);
        energy[(long)j * hw + p] = v;
    }
}

extern "C" int upsnet_mask_paste(void *stream, const float *mask_rois, const float *mask_logit, const int64_t *keep_inds,
                                 const int *num_keep, const int *real_keep, int kmax, int mask_size, int H, int W,
                                 float *mask_energy)
{
    UPS_REQUIRE(mask_rois && mask_logit && keep_inds && num_keep && real_keep && mask_energy, "mask_paste: null pointer");
    UPS_REQUIRE(kmax >= 1 && kmax <= 65535, "mask_paste: bad kmax");
    int gx = ups_divup((long)H * W, 256);
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(mask_paste_kernel, dim3(gx, kmax), dim3(256), 0, (hipStream_t)stream, mask_rois, mask_logit, keep_inds,
                       num_keep, real_keep, mask_size, H, W, mask_energy);
    UPS_CHECK_LAUNCH("mask_paste_kernel");
    return 0;
}

struct SegBox { int y0, y1, x0, x1; };
__device__ static inline int pan_py_slice(long v, int n) { if (v < 0) { v += n; if (v < 0) v = 0; } if (v > n) v = n; return (int)v; }
__device__ static inline SegBox pan_seg_box(float bx1, float by1, float bx2, float by2, int H, int W)
{
    SegBox s;  // unary_logits.py:99-102: int() truncates, numpy round is half-to-even
    s.y0 = pan_py_slice((long)by1, H); s.y1 = pan_py_slice((long)(rintf(by2) + 1.0f), H);
    s.x0 = pan_py_slice((long)bx1, W); s.x1 = pan_py_slice((long)(rintf(bx2) + 1.0f), W);
    return s;
}

__global__ void __launch_bounds__(256)
seg_term_kernel(const float *__restrict__ fcn, const int H, const int W, const float *__restrict__ boxes,
                const int64_t *__restrict__ cls, const int64_t *__restrict__ class_map, float *__restrict__ seg_inst)
{
    const int j = blockIdx.y;
    const long hw = (long)H * W;
    const int64_t c = cls[j];
    const SegBox s = pan_seg_box(boxes[j * 4 + 0], boxes[j * 4 + 1], boxes[j * 4 + 2], boxes[j * 4 + 3], H, W);
    const float *src = fcn + (c != 0 ? class_map[c] : 0) * hw;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long)blockDim.x * gridDim.x) {
        const int y = (int)(p / W), x = (int)(p % W);
        float v = 0.f;
        if (c != 0 && y >= s.y0 && y < s.y1 && x >= s.x0 && x < s.x1) v = src[p];
        seg_inst[(long)j * hw + p] = v;
    }
}

extern "C" int upsnet_seg_term(void *stream, const float *fcn_output, int num_seg, int H, int W, const float *boxes,
                               const int64_t *cls, const int64_t *class_map, int k, float *seg_inst)
{
    (void)num_seg;
    UPS_REQUIRE(fcn_output && boxes && cls && class_map && seg_inst, "seg_term: null pointer");
    UPS_REQUIRE(k >= 1 && k <= 65535, "seg_term: bad k");
    int gx = ups_divup((long)H * W, 256);
    if (gx > 2048) gx = 2048;
    hipLaunchKernelGGL(seg_term_kernel, dim3(gx, k), dim3(256), 0, (hipStream_t)stream, fcn_output, H, W, boxes, cls, class_map,
                       seg_inst);
    UPS_CHECK_LAUNCH("seg_term_kernel");
    return 0;
}

// reference-shaped fusion on materialised planes
__global__ void __launch_bounds__(256)
panoptic_argmax_kernel(const float *__restrict__ fcn, const int S, const long hw, const int s_stuff,
                       const float *__restrict__ seg_inst, const float *__restrict__ energy, const int k,
                       const int enable_void, int64_t *__restrict__ pan)
{
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < hw; p += (long)blockDim.x * gridDim.x) {
        float best = fcn[p];
        int bi = 0;
        for (int c = 1; c < s_stuff; ++c) { const float v = fcn[(long)c * hw + p]; if (v > best) { best = v; bi = c; } }
        if (enable_void) {
            float mi = seg_inst[p];
            for (int j = 0; j < k; ++j) {
                const float si = seg_inst[(long)j * hw + p];
                const float v = si + energy[(long)j * hw + p];
                if (v > best) { best = v; bi = s_stuff + j; }
                if (si > mi) mi = si;
            }
            float mt = fcn[(long)s_stuff * hw + p];
            for (int c = s_stuff + 1; c < S; ++c) { const float v = fcn[(long)c * hw + p]; if (v > mt) mt = v; }
            const float vd = mt - mi;
            pan[p] = vd > best ? 255 : bi;
        } else {
            // argmax(softmax(x)) restated explicitly (resnet_upsnet.py:242-243)
            float m = best;
            for (int j = 0; j < k; ++j) { const float v = seg_inst[(long)j * hw + p] + energy[(long)j * hw + p]; if (v > m) m = v; }
            float s = 0.f;
            for (int c = 0; c < s_stuff; ++c) s += ups_exp_f32(fcn[(long)c * hw + p] - m);
            for (int j = 0; j < k; ++j) s += ups_exp_f32(seg_inst[(long)j * hw + p] + energy[(long)j * hw + p] - m);
            float bp = ups_exp_f32(fcn[p] - m) / s;
            bi = 0;
            for (int c = 1; c < s_stuff; ++c) { const float pr = ups_exp_f32(fcn[(long)c * hw + p] - m) / s; if (pr > bp) { bp = pr; bi = c; } }
            for (int j = 0; j < k; ++j) {
                const float pr = ups_exp_f32(seg_inst[(long)j * hw + p] + energy[(long)j * hw + p] - m) / s;
                if (pr > bp) { bp = pr; bi = s_stuff + j; }
            }
            pan[p] = bi;
        }
    }
}

extern "C" int upsnet_panoptic_argmax(void *stream, const float *fcn_output, int num_seg, int H, int W, int num_stuff,
                                      const float *seg_inst, const float *mask_energy, int k, int enable_void, int64_t *pan_out)
{
    UPS_REQUIRE(fcn_output && seg_inst && mask_energy && pan_out, "panoptic_argmax: null pointer");
    UPS_REQUIRE(k >= 1 && num_stuff >= 1 && num_stuff < num_seg, "panoptic_argmax: bad k / channel split");
    const long hw = (long)H * W;
    int gx = ups_divup(hw, 256);
    if (gx > 8192) gx = 8192;
    hipLaunchKernelGGL(panoptic_argmax_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, fcn_output, num_seg, hw, num_stuff,
                       seg_inst, mask_energy, k, enable_void, pan_out);
    UPS_CHECK_LAUNCH("panoptic_argmax_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// fused head: one pass over fcn_output
#define FUSE_MAXK 256
struct FuseInst {
    PanBox mb;       // mask paste geometry
    SegBox sb;       // SegTerm crop
    int sem_ch;      // fcn channel of the instance class, -1 for the dummy (cls 0)
    int logit_off;   // offset of the 28x28 logits
};

template <int VEC>
__global__ void __launch_bounds__(256)
panoptic_fuse_kernel(const float *__restrict__ fcn, const int S, const int H, const int W, const int s_stuff,
                     const float *__restrict__ mask_rois, const float *__restrict__ logits, const int64_t *__restrict__ cls_idx,
                     const int64_t *__restrict__ keep_inds, const int *__restrict__ num_keep, const int *__restrict__ real_keep,
                     const int ms, const int64_t *__restrict__ class_map, const int enable_void, int64_t *__restrict__ pan,
                     int64_t *__restrict__ sem)
{
    __shared__ FuseInst s_inst[FUSE_MAXK];
    __shared__ int s_list[FUSE_MAXK];
    __shared__ int s_nlist;
    const int k = min(*num_keep, FUSE_MAXK);
    const bool real = *real_keep != 0;
    const long hw = (long)H * W;
    // tile of this workgroup: one image row, 256*VEC consecutive pixels
    const int tiles_per_row = (W + 256 * VEC - 1) / (256 * VEC);
    const int y = blockIdx.x / tiles_per_row;
    const int xt0 = (blockIdx.x % tiles_per_row) * 256 * VEC;
    const int xt1 = min(xt0 + 256 * VEC, W);
    if (threadIdx.x == 0) s_nlist = 0;
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const long i = keep_inds[j];
        const float *r = mask_rois + i * 5;
        FuseInst fi;
        fi.mb = pan_box(r + 1, H, W);
        // SegTerm sees mask_rois*4.0 (resnet_upsnet.py:227) times box_scale 1/4 (unary_logits.py:89)
        const float b0 = (r[1] * 4.0f) * 0.25f, b1 = (r[2] * 4.0f) * 0.25f, b2 = (r[3] * 4.0f) * 0.25f, b3 = (r[4] * 4.0f) * 0.25f;
        fi.sb = pan_seg_box(b0, b1, b2, b3, H, W);
        const int64_t c = cls_idx[i];
        fi.sem_ch = c != 0 ? (int)class_map[c] : -1;
        fi.logit_off = (int)(i * ms * ms);
        s_inst[j] = fi;
    }
    __syncthreads();
    // cull: instances that touch this row segment (kept in instance order by a serial pass of thread 0
    // over <= 256 flags computed in parallel)
    __shared__ unsigned char s_touch[FUSE_MAXK];
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const FuseInst &fi = s_inst[j];
        const bool tm = real && y >= fi.mb.y_0 && y < fi.mb.y_1 && fi.mb.x_0 < xt1 && fi.mb.x_1 > xt0;
        const bool ts = fi.sem_ch >= 0 && y >= fi.sb.y0 && y < fi.sb.y1 && fi.sb.x0 < xt1 && fi.sb.x1 > xt0;
        s_touch[j] = tm || ts;
    }
    __syncthreads();
    if (threadIdx.x == 0) { int n = 0; for (int j = 0; j < k; ++j) if (s_touch[j]) s_list[n++] = j; s_nlist = n; }
    __syncthreads();
    const int nlist = s_nlist;

    const int x0 = xt0 + threadIdx.x * VEC;
    if (x0 >= W) return;
    const long p0 = (long)y * W + x0;
    float v[VEC], best[VEC], tmax[VEC], sbest[VEC];
    int bi[VEC], sbi[VEC];
    // ---- stuff channels: running first-max
#pragma unroll
    for (int q = 0; q < VEC; ++q) { best[q] = 0.f; bi[q] = 0; }
    for (int c = 0; c < S; ++c) {
        if (VEC == 4) {
            const float4 t = *reinterpret_cast<const float4 *>(fcn + (long)c * hw + p0);
            v[0] = t.x; v[1 % VEC] = t.y; v[2 % VEC] = t.z; v[3 % VEC] = t.w;
        } else {
            v[0] = fcn[(long)c * hw + p0];
        }
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            if (c == 0) { best[q] = v[q]; bi[q] = 0; sbest[q] = v[q]; sbi[q] = 0; }
            else {
                if (c < s_stuff && v[q] > best[q]) { best[q] = v[q]; bi[q] = c; }
                if (v[q] > sbest[q]) { sbest[q] = v[q]; sbi[q] = c; }
            }
            if (c == s_stuff) tmax[q] = v[q];
            else if (c > s_stuff && v[q] > tmax[q]) tmax[q] = v[q];
        }
    }
    // ---- instance channels in order; untouched instances contribute logit 0 (and seg_inst 0)
    float mi[VEC];
    bool any_zero_before[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) { mi[q] = 0.f; any_zero_before[q] = false; }
    // mi starts from seg_inst of instance 0; instances not in the list have seg_inst == 0. Since k >= 1 the
    // maximum over all k planes is max(0 if any plane is 0 here, listed values). Track it exactly:
    float mi_listed[VEC];
    int n_nonzero_planes[VEC];
#pragma unroll
    for (int q = 0; q < VEC; ++q) { mi_listed[q] = -INFINITY; n_nonzero_planes[q] = 0; }
    int li = 0;
    for (int j = 0; j < k; ++j) {
        const bool listed = li < nlist && s_list[li] == j;
        if (listed) ++li;
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const int x = x0 + q;
            float si = 0.f, mk = 0.f;
            bool inseg = false;
            if (listed && x < W) {
                const FuseInst &fi = s_inst[j];
                if (fi.sem_ch >= 0 && y >= fi.sb.y0 && y < fi.sb.y1 && x >= fi.sb.x0 && x < fi.sb.x1) {
                    si = fcn[(long)fi.sem_ch * hw + (long)y * W + x];
                    inseg = true;
                }
                if (real && y >= fi.mb.y_0 && y < fi.mb.y_1 && x >= fi.mb.x_0 && x < fi.mb.x_1)
                    mk = pan_resize_at(logits + fi.logit_off, ms, fi.mb.w, fi.mb.h, x - fi.mb.bx0, y - fi.mb.by0);
            }
            const float inst = si + mk;
            if (inst > best[q]) { best[q] = inst; bi[q] = s_stuff + j; }
            if (inseg) { if (si > mi_listed[q]) mi_listed[q] = si; ++n_nonzero_planes[q]; }
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        // max_j seg_inst_j: planes where the pixel is outside the SegTerm crop hold exactly 0
        float m = mi_listed[q];
        if (n_nonzero_planes[q] < k) m = fmaxf(m, 0.f);
        mi[q] = m;
        (void)any_zero_before[q];
    }
    if (!enable_void) {
        // argmax(softmax(.)) variant: recompute with explicit softmax (rare path: keep_fraction >= 1)
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            const int x = x0 + q;
            if (x >= W) continue;
            const long p = (long)y * W + x;
            float m = best[q];
            float s = 0.f;
            for (int c = 0; c < s_stuff; ++c) s += ups_exp_f32(fcn[(long)c * hw + p] - m);
            int lj = 0;
            for (int j = 0; j < k; ++j) {
                const bool listed = lj < nlist && s_list[lj] == j;
                if (listed) ++lj;
                float si = 0.f, mk = 0.f;
                if (listed) {
                    const FuseInst &fi = s_inst[j];
                    if (fi.sem_ch >= 0 && y >= fi.sb.y0 && y < fi.sb.y1 && x >= fi.sb.x0 && x < fi.sb.x1) si = fcn[(long)fi.sem_ch * hw + p];
                    if (real && y >= fi.mb.y_0 && y < fi.mb.y_1 && x >= fi.mb.x_0 && x < fi.mb.x_1)
                        mk = pan_resize_at(logits + fi.logit_off, ms, fi.mb.w, fi.mb.h, x - fi.mb.bx0, y - fi.mb.by0);
                }
                s += ups_exp_f32(si + mk - m);
            }
            float bp = ups_exp_f32(fcn[p] - m) / s;
            int b2 = 0;
            for (int c = 1; c < s_stuff; ++c) { const float pr = ups_exp_f32(fcn[(long)c * hw + p] - m) / s; if (pr > bp) { bp = pr; b2 = c; } }
            lj = 0;
            for (int j = 0; j < k; ++j) {
                const bool listed = lj < nlist && s_list[lj] == j;
                if (listed) ++lj;
                float si = 0.f, mk = 0.f;
                if (listed) {
                    const FuseInst &fi = s_inst[j];
                    if (fi.sem_ch >= 0 && y >= fi.sb.y0 && y < fi.sb.y1 && x >= fi.sb.x0 && x < fi.sb.x1) si = fcn[(long)fi.sem_ch * hw + p];
                    if (real && y >= fi.mb.y_0 && y < fi.mb.y_1 && x >= fi.mb.x_0 && x < fi.mb.x_1)
                        mk = pan_resize_at(logits + fi.logit_off, ms, fi.mb.w, fi.mb.h, x - fi.mb.bx0, y - fi.mb.by0);
                }
                const float pr = ups_exp_f32(si + mk - m) / s;
                if (pr > bp) { bp = pr; b2 = s_stuff + j; }
            }
            bi[q] = b2;
        }
    }
#pragma unroll
    for (int q = 0; q < VEC; ++q) {
        const int x = x0 + q;
        if (x >= W) continue;
        int64_t lab = bi[q];
        if (enable_void) { const float vd = tmax[q] - mi[q]; if (vd > best[q]) lab = 255; }
        pan[(long)y * W + x] = lab;
        if (sem) sem[(long)y * W + x] = sbi[q];
    }
}

extern "C" int upsnet_panoptic_fuse(void *stream, const float *fcn_output, int num_seg, int H, int W, int num_stuff,
                                    const float *mask_rois, const float *mask_logit, const int64_t *cls_idx,
                                    const int64_t *keep_inds, const int *num_keep, const int *real_keep, int kmax,
                                    int mask_size, const int64_t *class_map, int enable_void, int64_t *pan_out,
                                    int64_t *sem_out)
{
    UPS_REQUIRE(fcn_output && mask_rois && mask_logit && cls_idx && keep_inds && num_keep && real_keep && class_map && pan_out,
                "panoptic_fuse: null pointer");
    UPS_REQUIRE(num_stuff >= 1 && num_stuff < num_seg, "panoptic_fuse: bad channel split %d/%d", num_stuff, num_seg);
    UPS_REQUIRE(kmax >= 1 && kmax <= FUSE_MAXK, "panoptic_fuse: at most %d instances supported (got %d)", FUSE_MAXK, kmax);
    UPS_REQUIRE(mask_size >= 2 && mask_size <= PAN_MAXMS, "panoptic_fuse: bad mask size");
    hipStream_t st = (hipStream_t)stream;
    if ((W & 3) == 0 && (((uintptr_t)fcn_output) & 15) == 0) {
        const int tiles = ((W + 1023) / 1024) * H;
        hipLaunchKernelGGL(panoptic_fuse_kernel<4>, dim3(tiles), dim3(256), 0, st, fcn_output, num_seg, H, W, num_stuff, mask_rois,
                           mask_logit, cls_idx, keep_inds, num_keep, real_keep, mask_size, class_map, enable_void, pan_out, sem_out);
    } else {
        const int tiles = ((W + 255) / 256) * H;
        hipLaunchKernelGGL(panoptic_fuse_kernel<1>, dim3(tiles), dim3(256), 0, st, fcn_output, num_seg, H, W, num_stuff, mask_rois,
                           mask_logit, cls_idx, keep_inds, num_keep, real_keep, mask_size, class_map, enable_void, pan_out, sem_out);
    }
    UPS_CHECK_LAUNCH("panoptic_fuse_kernel");
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Fused head, variant that ALSO fuses the x`scale` bilinear upsampling of the semantic logits
// (F.interpolate(score, None, 4, 'bilinear', align_corners=False), upsnet/models/fcn.py:101): reads the
// low-resolution fcn_score (10 MB at C1) instead of a materialised 159 MB fcn_output. A workgroup owns a
// 128 x 8 output tile; its (128/scale + 2) x (8/scale + 2) x S source patch is staged in LDS as [c][sy][sx];
// every logit is re-interpolated from LDS with PyTorch's upsample_bilinear2d arithmetic restated in fp32
// without FMA (bit-identical to oracle/c: orc_upsample_bilinear).
#define FUP_TW 128
#define FUP_TH 8
#define FUP_MAXS 160      // max semantic classes (133 for COCO)

struct UpCoef { int i0, ip; float l0, l1; };
__device__ static inline UpCoef fup_coef(int dst, float r, int src_size)
{
    UpCoef c;
    float s = r * ((float)dst + 0.5f) - 0.5f;
    if (s < 0) s = 0;
    c.i0 = (int)s;
    c.ip = c.i0 < src_size - 1 ? 1 : 0;
    c.l1 = s - (float)c.i0;
    c.l0 = 1.0f - c.l1;
    return c;
}

// The body of both kernels below. CONF: also the confidence of the winner (include/upsnet_hip.h: upsnet_panoptic_fuse_up_conf), one
// byte per pixel into `conf`; without it `conf` is never touched and every CONF statement folds away (profiles/pan_confidence.txt: the
// label-only kernel's registers, LDS and occupancy are what they were before the body was shared).
template <int SCALE, bool CONF>
__device__ __forceinline__ void
fup_tile(const float *__restrict__ score, const long pix_stride, const long ch_stride, const int S, const int Hs, const int Ws,
         const int s_stuff, const float *__restrict__ mask_rois, const float *__restrict__ logits, const int64_t *__restrict__ cls_idx,
         const int64_t *__restrict__ keep_inds, const int *__restrict__ num_keep, const int *__restrict__ real_keep, const int ms,
         const int64_t *__restrict__ class_map, const int enable_void, int64_t *__restrict__ pan, int64_t *__restrict__ sem,
         unsigned char *__restrict__ conf)
{
    constexpr int SW = FUP_TW / SCALE + 2, SH = FUP_TH / SCALE + 2;  // source patch incl. halo
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float *s_src = reinterpret_cast<float *>(smem_raw);                        // [S][SH][SW]
    FuseInst *s_inst = reinterpret_cast<FuseInst *>(s_src + (size_t)S * SH * SW);  // [FUSE_MAXK]
    int *s_list = reinterpret_cast<int *>(s_inst + FUSE_MAXK);
    unsigned char *s_touch = reinterpret_cast<unsigned char *>(s_list + FUSE_MAXK);
    __shared__ int s_nlist, s_first_unlisted;

    const int H = Hs * SCALE, W = Ws * SCALE;
    const long hw = (long)H * W;
    (void)hw;
    const int tiles_x = (W + FUP_TW - 1) / FUP_TW;
    const int ty0 = (blockIdx.x / tiles_x) * FUP_TH, tx0 = (blockIdx.x % tiles_x) * FUP_TW;
    const int ty1 = min(ty0 + FUP_TH, H), tx1 = min(tx0 + FUP_TW, W);
    const int k = min(*num_keep, FUSE_MAXK);
    const bool real = *real_keep != 0;
    const float r = 1.0f / (float)SCALE;

    // ---- source patch origin: the first source row/col any pixel of the tile touches
    const int sy0 = fup_coef(ty0, r, Hs).i0, sx0 = fup_coef(tx0, r, Ws).i0;
    for (int idx = threadIdx.x; idx < S * SH * SW; idx += blockDim.x) {
        const int c = idx % S, rest = idx / S;   // channel fastest: coalesced for NHWC score
        const int sx = rest % SW, sy = rest / SW;
        const int gy = min(sy0 + sy, Hs - 1), gx = min(sx0 + sx, Ws - 1);
        s_src[(c * SH + sy) * SW + sx] = score[((long)gy * Ws + gx) * pix_stride + (long)c * ch_stride];
    }
    if (threadIdx.x == 0) s_nlist = 0;
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const long i = keep_inds[j];
        const float *rr = mask_rois + i * 5;
        FuseInst fi;
        fi.mb = pan_box(rr + 1, H, W);
        const float b0 = (rr[1] * 4.0f) * 0.25f, b1 = (rr[2] * 4.0f) * 0.25f, b2 = (rr[3] * 4.0f) * 0.25f, b3 = (rr[4] * 4.0f) * 0.25f;
        fi.sb = pan_seg_box(b0, b1, b2, b3, H, W);
        const int64_t c = cls_idx[i];
        fi.sem_ch = c != 0 ? (int)class_map[c] : -1;
        fi.logit_off = (int)(i * ms * ms);
        s_inst[j] = fi;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        const FuseInst &fi = s_inst[j];
        const bool tm = real && fi.mb.y_0 < ty1 && fi.mb.y_1 > ty0 && fi.mb.x_0 < tx1 && fi.mb.x_1 > tx0;
        const bool ts = fi.sem_ch >= 0 && fi.sb.y0 < ty1 && fi.sb.y1 > ty0 && fi.sb.x0 < tx1 && fi.sb.x1 > tx0;
        s_touch[j] = tm || ts;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0, u0 = k;
        for (int j = 0; j < k; ++j) { if (s_touch[j]) s_list[n++] = j; else if (u0 == k) u0 = j; }
        s_nlist = n; s_first_unlisted = u0;
    }
    __syncthreads();
    const int nlist = s_nlist, u0 = s_first_unlisted;

    // thread -> 4 consecutive pixels of one tile row
    const int y = ty0 + threadIdx.x / (FUP_TW / 4);
    const int x0 = tx0 + (threadIdx.x % (FUP_TW / 4)) * 4;
    if (y >= H || x0 >= W) return;
    const UpCoef cy = fup_coef(y, r, Hs);
    UpCoef cx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) cx[q] = fup_coef(min(x0 + q, W - 1), r, Ws);
    const int ly0 = cy.i0 - sy0, ly1 = ly0 + cy.ip;

#define FUP_AT(C, Q)                                                                                              \
    (cy.l0 * (cx[Q].l0 * s_src[((C) * SH + ly0) * SW + cx[Q].i0 - sx0] + cx[Q].l1 * s_src[((C) * SH + ly0) * SW + cx[Q].i0 - sx0 + cx[Q].ip]) + \
     cy.l1 * (cx[Q].l0 * s_src[((C) * SH + ly1) * SW + cx[Q].i0 - sx0] + cx[Q].l1 * s_src[((C) * SH + ly1) * SW + cx[Q].i0 - sx0 + cx[Q].ip]))

    float best[4], tmax[4], sbest[4];
    int bi[4], sbi[4];
    for (int c = 0; c < S; ++c) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float v = FUP_AT(c, q);
            if (c == 0) { best[q] = v; bi[q] = 0; sbest[q] = v; sbi[q] = 0; }
            else {
                if (c < s_stuff && v > best[q]) { best[q] = v; bi[q] = c; }
                if (v > sbest[q]) { sbest[q] = v; sbi[q] = c; }
            }
            if (c == s_stuff) tmax[q] = v;
            else if (c > s_stuff && v > tmax[q]) tmax[q] = v;
        }
    }
    float mi_listed[4];
    int n_in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { mi_listed[q] = -INFINITY; n_in[q] = 0; }
    // Instances in index order (first maximum wins, resnet_upsnet.py:241-243). An instance that touches this tile nowhere has the
    // logit 0 at every pixel of it; of all those only the FIRST (index u0) can ever become the arg-max (the others are not strictly
    // greater), so the loop visits the touching instances only and drops the one zero candidate in at its place in the order --
    // O(instances touching the tile) per pixel instead of O(k).
    bool zero_done = u0 >= k;
    for (int li = 0; li <= nlist; ++li) {
        const int j = li < nlist ? s_list[li] : k;
        if (!zero_done && u0 < j) {
#pragma unroll
            for (int q = 0; q < 4; ++q) if (0.f > best[q]) { best[q] = 0.f; bi[q] = s_stuff + u0; }
            zero_done = true;
        }
        if (li == nlist) break;
        const FuseInst &fi = s_inst[j];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = x0 + q;
            float si = 0.f, mk = 0.f;
            bool inseg = false;
            if (x < W) {
                if (fi.sem_ch >= 0 && y >= fi.sb.y0 && y < fi.sb.y1 && x >= fi.sb.x0 && x < fi.sb.x1) { si = FUP_AT(fi.sem_ch, q); inseg = true; }
                if (real && y >= fi.mb.y_0 && y < fi.mb.y_1 && x >= fi.mb.x_0 && x < fi.mb.x_1)
                    mk = pan_resize_at(logits + fi.logit_off, ms, fi.mb.w, fi.mb.h, x - fi.mb.bx0, y - fi.mb.by0);
            }
            const float inst = si + mk;
            if (inst > best[q]) { best[q] = inst; bi[q] = s_stuff + j; }
            if (inseg) { if (si > mi_listed[q]) mi_listed[q] = si; ++n_in[q]; }
        }
    }
    float zmax[4], zvoid[4];   // CONF: the winner's logit and the void logit
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int x = x0 + q;
        if (CONF) { zmax[q] = best[q]; zvoid[q] = best[q]; }
        if (x >= W) continue;
        float m = mi_listed[q];
        if (n_in[q] < k) m = fmaxf(m, 0.f);
        int64_t lab = bi[q];
        if (enable_void) {
            const float vd = tmax[q] - m;
            if (vd > best[q]) lab = 255;
            if (CONF) { zvoid[q] = vd; zmax[q] = fmaxf(best[q], vd); }
        }
        pan[(long)y * W + x] = lab;
        if (sem) sem[(long)y * W + x] = sbi[q];
    }
    if (CONF) {
        // conf = P[winner] = 1 / sum_c exp(z_c - z_max) over the stuff channels, ALL k instance channels and the void channel: a second
        // walk over the same logits now that z_max is known (every term <= 1, the winner's is exactly 1). The first-zero shortcut of
        // the arg-max does not carry over: each of the k - nlist instances that touch the tile nowhere has the logit 0 and adds
        // exp(0 - z_max), the same term, added once with its count.
        float sum[4] = {0.f, 0.f, 0.f, 0.f};
        for (int c = 0; c < s_stuff; ++c) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[q] += __expf(FUP_AT(c, q) - zmax[q]);
        }
        for (int li = 0; li < nlist; ++li) {
            const FuseInst &fi = s_inst[s_list[li]];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int x = x0 + q;
                float si = 0.f, mk = 0.f;
                if (x < W) {
                    if (fi.sem_ch >= 0 && y >= fi.sb.y0 && y < fi.sb.y1 && x >= fi.sb.x0 && x < fi.sb.x1) si = FUP_AT(fi.sem_ch, q);
                    if (real && y >= fi.mb.y_0 && y < fi.mb.y_1 && x >= fi.mb.x_0 && x < fi.mb.x_1)
                        mk = pan_resize_at(logits + fi.logit_off, ms, fi.mb.w, fi.mb.h, x - fi.mb.bx0, y - fi.mb.by0);
                }
                sum[q] += __expf((si + mk) - zmax[q]);
            }
        }
        const float untouched = (float)(k - nlist);
        unsigned packed = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (k > nlist) sum[q] += untouched * __expf(0.f - zmax[q]);
            if (enable_void) sum[q] += __expf(zvoid[q] - zmax[q]);
            const float c = 1.0f / sum[q];
            packed |= ((unsigned)(c * 255.0f + 0.5f) & 255u) << (8 * q);
        }
        // W = 4 Ws and x0 are multiples of 4 (and `conf` 4-byte aligned): the thread's four bytes are one aligned word, all inside the row
        *reinterpret_cast<unsigned *>(conf + (long)y * W + x0) = packed;
    }
#undef FUP_AT
}

template <int SCALE>
__global__ void __launch_bounds__(256)
panoptic_fuse_up_kernel(const float *__restrict__ score, const long pix_stride, const long ch_stride, const int S,
                        const int Hs, const int Ws, const int s_stuff, const float *__restrict__ mask_rois,
                        const float *__restrict__ logits, const int64_t *__restrict__ cls_idx,
                        const int64_t *__restrict__ keep_inds, const int *__restrict__ num_keep,
                        const int *__restrict__ real_keep, const int ms, const int64_t *__restrict__ class_map,
                        const int enable_void, int64_t *__restrict__ pan, int64_t *__restrict__ sem)
{
    fup_tile<SCALE, false>(score, pix_stride, ch_stride, S, Hs, Ws, s_stuff, mask_rois, logits, cls_idx, keep_inds, num_keep, real_keep, ms,
                           class_map, enable_void, pan, sem, nullptr);
}

// The sibling with the confidence plane: a separate kernel, so that the label-only one keeps its registers and its occupancy.
template <int SCALE>
__global__ void __launch_bounds__(256)
panoptic_fuse_up_conf_kernel(const float *__restrict__ score, const long pix_stride, const long ch_stride, const int S,
                             const int Hs, const int Ws, const int s_stuff, const float *__restrict__ mask_rois,
                             const float *__restrict__ logits, const int64_t *__restrict__ cls_idx,
                             const int64_t *__restrict__ keep_inds, const int *__restrict__ num_keep,
                             const int *__restrict__ real_keep, const int ms, const int64_t *__restrict__ class_map,
                             const int enable_void, int64_t *__restrict__ pan, int64_t *__restrict__ sem,
                             unsigned char *__restrict__ conf)
{
    fup_tile<SCALE, true>(score, pix_stride, ch_stride, S, Hs, Ws, s_stuff, mask_rois, logits, cls_idx, keep_inds, num_keep, real_keep, ms,
                          class_map, enable_void, pan, sem, conf);
}

// both entry points: `name` words the errors; conf_out == nullptr launches the label-only kernel
static int fup_launch(const char *name, void *stream, const float *fcn_score, int score_nhwc, int num_seg, int score_h, int score_w,
                      int scale, int num_stuff, const float *mask_rois, const float *mask_logit, const int64_t *cls_idx,
                      const int64_t *keep_inds, const int *num_keep, const int *real_keep, int kmax, int mask_size,
                      const int64_t *class_map, int64_t *pan_out, int64_t *sem_out, unsigned char *conf_out)
{
    UPS_REQUIRE(fcn_score && mask_rois && mask_logit && cls_idx && keep_inds && num_keep && real_keep && class_map && pan_out,
                "%s: null pointer", name);
    UPS_REQUIRE(scale == 4, "%s: only the x4 upsampling of FCNHead (upsample_rate=4) is built (got %d)", name, scale);
    UPS_REQUIRE(num_stuff >= 1 && num_stuff < num_seg && num_seg <= FUP_MAXS, "%s: bad channel split %d/%d", name, num_stuff, num_seg);
    UPS_REQUIRE(kmax >= 1 && kmax <= FUSE_MAXK, "%s: at most %d instances supported (got %d)", name, FUSE_MAXK, kmax);
    UPS_REQUIRE(mask_size >= 2 && mask_size <= PAN_MAXMS, "%s: bad mask size", name);
    const int H = score_h * scale, W = score_w * scale;
    const int tiles = ((W + FUP_TW - 1) / FUP_TW) * ((H + FUP_TH - 1) / FUP_TH);
    const size_t smem = (size_t)num_seg * (FUP_TH / 4 + 2) * (FUP_TW / 4 + 2) * sizeof(float) + FUSE_MAXK * (sizeof(FuseInst) + sizeof(int) + 1) + 16;
    const long pix_stride = score_nhwc ? num_seg : 1, ch_stride = score_nhwc ? 1 : (long)score_h * score_w;
    static std::atomic<unsigned long long> attr_dev{0}, attr_dev_conf{0};
    if (conf_out) {
        if (smem > 64 * 1024)
            UPS_ONCE_PER_DEVICE(attr_dev_conf, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&panoptic_fuse_up_conf_kernel<4>),
                                                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)));
        hipLaunchKernelGGL(panoptic_fuse_up_conf_kernel<4>, dim3(tiles), dim3(256), smem, (hipStream_t)stream, fcn_score, pix_stride,
                           ch_stride, num_seg, score_h, score_w, num_stuff, mask_rois, mask_logit, cls_idx, keep_inds, num_keep, real_keep,
                           mask_size, class_map, 1, pan_out, sem_out, conf_out);
        UPS_CHECK_LAUNCH("panoptic_fuse_up_conf_kernel");
        return 0;
    }
    if (smem > 64 * 1024)
        UPS_ONCE_PER_DEVICE(attr_dev, UPS_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(&panoptic_fuse_up_kernel<4>),
                                                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem)));
    hipLaunchKernelGGL(panoptic_fuse_up_kernel<4>, dim3(tiles), dim3(256), smem, (hipStream_t)stream, fcn_score, pix_stride, ch_stride,
                       num_seg, score_h, score_w, num_stuff, mask_rois, mask_logit, cls_idx, keep_inds, num_keep, real_keep, mask_size,
                       class_map, 1, pan_out, sem_out);
    UPS_CHECK_LAUNCH("panoptic_fuse_up_kernel");
    return 0;
}

extern "C" int upsnet_panoptic_fuse_up(void *stream, const float *fcn_score, int score_nhwc, int num_seg, int score_h, int score_w,
                                       int scale, int num_stuff, const float *mask_rois, const float *mask_logit,
                                       const int64_t *cls_idx, const int64_t *keep_inds, const int *num_keep, const int *real_keep,
                                       int kmax, int mask_size, const int64_t *class_map, int64_t *pan_out, int64_t *sem_out)
{
    return fup_launch("panoptic_fuse_up", stream, fcn_score, score_nhwc, num_seg, score_h, score_w, scale, num_stuff, mask_rois, mask_logit,
                      cls_idx, keep_inds, num_keep, real_keep, kmax, mask_size, class_map, pan_out, sem_out, nullptr);
}

extern "C" int upsnet_panoptic_fuse_up_conf(void *stream, const float *fcn_score, int score_nhwc, int num_seg, int score_h, int score_w,
                                            int scale, int num_stuff, const float *mask_rois, const float *mask_logit,
                                            const int64_t *cls_idx, const int64_t *keep_inds, const int *num_keep, const int *real_keep,
                                            int kmax, int mask_size, const int64_t *class_map, int64_t *pan_out, int64_t *sem_out,
                                            unsigned char *conf_out)
{
    UPS_REQUIRE(conf_out && ((uintptr_t)conf_out & 3) == 0, "panoptic_fuse_up_conf: conf_out null or not 4-byte aligned");
    return fup_launch("panoptic_fuse_up_conf", stream, fcn_score, score_nhwc, num_seg, score_h, score_w, scale, num_stuff, mask_rois,
                      mask_logit, cls_idx, keep_inds, num_keep, real_keep, kmax, mask_size, class_map, pan_out, sem_out, conf_out);
}

