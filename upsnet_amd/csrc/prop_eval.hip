// prop_eval.hip -- BaseDataset.evaluate_box_proposals (upsnet/dataset/base_dataset.py:723-805), the per-image part: the greedy
// one-to-one matching of proposals to GT boxes whose recorded IoUs make Detectron's average recall.
//
// A problem is (image, GT subset of one area range, proposal prefix cut to one limit); the host (dataset/proposal_eval.py) does the
// selection with the reference's numpy expressions and packs every problem of an image into one launch. One workgroup per problem:
//   * IoU = bbox_overlaps_c of upsnet/bbox/bbox.pyx, fp32 in its operation order (-ffp-contract=off, correctly rounded division);
//     the P x G matrix is never stored, every value is recomputed when needed (bit-identical by construction);
//   * per GT column c, in LDS: key = (bits(max IoU over the alive rows) << 32) | ~argmax row. IoUs are >= +0, so the bit pattern
//     orders like the value and the 64-bit max picks the largest IoU, then the FIRST row among equal ones (numpy argmax, axis 0);
//     key 0 marks a deleted column (a live key has ~row != 0 in its low word);
//   * alive rows: one bit per proposal in the workspace, written by the kernel before it is read;
//   * step j: workgroup argmax over the alive columns with the key (bits(max) << 32) | ~column (max_overlaps.argmax(): the first
//     column among equal maxima), record the IoU, delete that row and column. Columns whose argmax row was deleted look for the first
//     alive row after it with the same IoU (rows before it hold smaller values, so that row is the new argmax); only when there is
//     none do they rescan all alive rows. One wave per column in both scans.
// Deleted rows / columns hold -1 in the reference; while j < min(P, G) an alive row and an alive column always exist, so "first
// alive index with the largest value" is the reference's choice. GT rows left unmatched (P < G) stay 0.
#include "common.h"
#include "upsnet_hip.h"

#define PR_BT 256                       // threads per workgroup (4 waves)
#define PR_NW (PR_BT / UPS_WAVE)
#define PR_MAX_GT 4096                  // GT boxes per problem (LDS: 8 + 4 bytes per column)
#define PR_COLS 6                       // problem table row: proposal offset, proposals, GT offset, GTs, output offset, word offset

typedef unsigned long long pr_u64;

// bbox_overlaps_c (bbox.pyx): b = proposal (boxes[n]), q = GT (query_boxes[k]), qarea = its box_area
__device__ static inline float pr_iou(const float4 b, const float4 q, const float qarea)
{
    const float iw = fminf(b.z, q.z) - fmaxf(b.x, q.x) + 1.0f;
    if (iw > 0.0f) {
        const float ih = fminf(b.w, q.w) - fmaxf(b.y, q.y) + 1.0f;
        if (ih > 0.0f) {
            const float ua = (b.z - b.x + 1.0f) * (b.w - b.y + 1.0f) + qarea - iw * ih;
            return iw * ih / ua;
        }
    }
    return 0.0f;
}

__device__ static inline float pr_area(const float4 q) { return (q.z - q.x + 1.0f) * (q.w - q.y + 1.0f); }

__device__ static inline pr_u64 pr_wave_max(pr_u64 v)
{
    for (int o = UPS_WAVE / 2; o > 0; o >>= 1) {
        const pr_u64 u = __shfl_xor(v, o, UPS_WAVE);
        v = u > v ? u : v;
    }
    return v;
}

__device__ static inline bool pr_alive(const unsigned *alive, const int r) { return (alive[r >> 5] >> (r & 31)) & 1u; }

__device__ static inline pr_u64 pr_key(const float v, const int r)
{
    return ((pr_u64)__float_as_uint(v) << 32) | (pr_u64)(0xFFFFFFFFu - (unsigned)r);
}

// Whole-wave scan of column q over the alive rows [r0, P): the largest key (0 if no row is alive).
__device__ static inline pr_u64 pr_scan(const float4 *__restrict__ props, const unsigned *alive, const int r0, const int P,
                                        const float4 q, const float qarea, const int lane)
{
    pr_u64 best = 0;
    for (int r = r0 + lane; r < P; r += UPS_WAVE) {
        if (!pr_alive(alive, r)) continue;
        const pr_u64 k = pr_key(pr_iou(props[r], q, qarea), r);
        best = k > best ? k : best;
    }
    return pr_wave_max(best);
}

// table int64 [num_problems][PR_COLS]; props float [.,4]; gts float [.,4]; out float [sum of GTs]; alive_all uint32 words
__global__ void __launch_bounds__(PR_BT)
prop_recall_kernel(const int64_t *__restrict__ table, const float4 *__restrict__ props_all, const float4 *__restrict__ gts_all,
                   float *__restrict__ out_all, unsigned *__restrict__ alive_all)
{
    __shared__ pr_u64 s_key[PR_MAX_GT];
    __shared__ int s_list[PR_MAX_GT];
    __shared__ pr_u64 s_wave[PR_NW];
    __shared__ int s_nlist;
    const int64_t *t = table + (long)blockIdx.x * PR_COLS;
    const float4 *props = props_all + t[0];
    const int P = (int)t[1];
    const float4 *gts = gts_all + t[2];
    const int G = (int)t[3];
    float *out = out_all + t[4];
    unsigned *alive = alive_all + t[5];
    const int tid = threadIdx.x, lane = tid & (UPS_WAVE - 1), wave = tid / UPS_WAVE;
    // a row outside the contract (the host validates the table; this keeps a wrong one inside LDS): nothing is read or written
    if (P < 0 || G < 0 || G > PR_MAX_GT) return;
    const int steps = min(P, G);
    for (int j = steps + tid; j < G; j += PR_BT) out[j] = 0.0f;
    if (steps == 0) return;
    const int words = (P + 31) >> 5;
    for (int w = tid; w < words; w += PR_BT) alive[w] = 0xFFFFFFFFu;
    __syncthreads();
    for (int c = wave; c < G; c += PR_NW) {
        const float4 q = gts[c];
        const pr_u64 k = pr_scan(props, alive, 0, P, q, pr_area(q), lane);
        if (lane == 0) s_key[c] = k;
    }
    __syncthreads();
    for (int j = 0; j < steps; ++j) {
        // (A) the best covered alive column: largest max IoU, then the first column
        pr_u64 best = 0;
        for (int c = tid; c < G; c += PR_BT) {
            const pr_u64 k = s_key[c];
            if (k == 0) continue;
            const pr_u64 kc = (k & 0xFFFFFFFF00000000ull) | (pr_u64)(0xFFFFFFFFu - (unsigned)c);
            best = kc > best ? kc : best;
        }
        best = pr_wave_max(best);
        if (lane == 0) s_wave[wave] = best;
        if (tid == 0) s_nlist = 0;
        __syncthreads();
        // (B) record it; list the alive columns whose argmax row is the deleted one
        best = s_wave[0];
        for (int w = 1; w < PR_NW; ++w) best = s_wave[w] > best ? s_wave[w] : best;
        const int g = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFu));
        const pr_u64 kg = s_key[g];
        const int box = (int)(0xFFFFFFFFu - (unsigned)(kg & 0xFFFFFFFFu));
        if (j + 1 == steps) {
            if (tid == 0) out[j] = __uint_as_float((unsigned)(kg >> 32));
            break;
        }
        for (int c = tid; c < G; c += PR_BT) {
            const pr_u64 k = s_key[c];
            if (c != g && k != 0 && (int)(0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFu)) == box) s_list[atomicAdd(&s_nlist, 1)] = c;
        }
        if (tid == 0) {
            out[j] = __uint_as_float((unsigned)(kg >> 32));
            alive[box >> 5] &= ~(1u << (box & 31));
        }
        __syncthreads();
        // (C) delete column g; new argmax for the listed columns
        if (tid == 0) s_key[g] = 0;
        const int nl = s_nlist;
        for (int i = wave; i < nl; i += PR_NW) {
            const int c = s_list[i];
            const pr_u64 old = s_key[c];
            const float v = __uint_as_float((unsigned)(old >> 32));
            const float4 q = gts[c];
            const float qa = pr_area(q);
            pr_u64 k = 0;
            for (int r0 = box + 1; r0 < P && k == 0; r0 += UPS_WAVE) {
                const int r = r0 + lane;
                const bool hit = r < P && pr_alive(alive, r) && pr_iou(props[r], q, qa) == v;
                const pr_u64 m = __ballot(hit);
                if (m) k = pr_key(v, r0 + (__ffsll((long long)m) - 1));
            }
            if (k == 0) k = pr_scan(props, alive, 0, P, q, qa, lane);
            if (lane == 0) s_key[c] = k;
        }
        __syncthreads();
    }
}

static inline size_t pr_align(size_t n) { return (n + 255) & ~(size_t)255; }

extern "C" size_t upsnet_proposal_recall_workspace_bytes(int num_problems, long total_proposals)
{
    if (num_problems <= 0 || total_proposals < 0) return 0;
    return pr_align(((size_t)total_proposals / 32 + (size_t)num_problems) * sizeof(unsigned));
}

extern "C" int upsnet_proposal_recall(void *stream, int num_problems, const int64_t *problems, const float *proposals,
                                      const float *gt_boxes, int max_gt, long total_proposals, void *workspace, float *out)
{
    UPS_REQUIRE(num_problems >= 0 && num_problems <= 65535, "proposal_recall: %d problems in one call (0..65535)", num_problems);
    if (num_problems == 0) return 0;
    UPS_REQUIRE(problems && proposals && gt_boxes && workspace && out, "proposal_recall: null pointer");
    UPS_REQUIRE(max_gt >= 0 && max_gt <= PR_MAX_GT, "proposal_recall: %d GT boxes in a problem (at most %d)", max_gt, PR_MAX_GT);
    UPS_REQUIRE(total_proposals >= 0 && total_proposals <= 0x7FFFFFFFL, "proposal_recall: %ld proposals in one call (at most 2^31 - 1)",
                total_proposals);
    UPS_REQUIRE(((uintptr_t)proposals & 15) == 0 && ((uintptr_t)gt_boxes & 15) == 0, "proposal_recall: boxes must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(prop_recall_kernel, dim3((unsigned)num_problems), dim3(PR_BT), 0, st, problems, (const float4 *)proposals,
                       (const float4 *)gt_boxes, out, (unsigned *)workspace);
    UPS_CHECK_LAUNCH("prop_recall_kernel");
    return 0;
}
