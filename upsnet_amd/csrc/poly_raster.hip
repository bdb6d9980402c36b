// poly_raster.hip -- polygon ground truth to run-length masks on the device: pycocotools' rleFrPoly (frPyObjects of a polygon list)
// followed by merge (union), i.e. COCO.annToRLE of a polygon annotation, restated from the published algorithm. All polygon objects
// of one image in one call; the result is what det_eval.hip takes for GT masks: per object the ascending column-major positions
// (x * h + y) where the mask value changes, the first one starting a run of ones.
//
// rleFrPoly upsamples the vertices by 5, walks every edge with max(|dX|, |dY|) + 1 points, emits a position wherever the walk's x
// changes on a pixel-centre column, sorts the positions and folds equal ones pairwise: a position survives iff it was emitted an odd
// number of times. The kernels, in stream order (no host synchronisation, everything in the caller's workspace):
//   pr_vertex_kernel   one thread per vertex: the upsampled integer vertex and the point count of the edge that starts at it
//   scan (3 kernels)   exclusive prefix over the edge point counts -> the first point of every edge (and of every polygon)
//   pr_emit_kernel     one thread per point: the point and its predecessor recomputed from their edge, the position or a sentinel,
//                      written as the 64-bit key (polygon << 32 | position); the array is padded to a power of two with ~0
//   bitonic sort       pr_sort_lds_kernel sorts runs of PR_CH keys in LDS, pr_sort_step_kernel does the compare-exchange steps whose
//                      stride does not fit a run in global memory, pr_sort_lds_kernel again finishes each stage in LDS: any
//                      length the workspace admits. Keys of one polygon stay inside that polygon's range of points, sentinels last.
//   pr_parity_kernel   the first key of every run of equal keys is flagged iff the run length is odd; scan -> rank
//   pr_union_kernel    objects of several polygons: coverage before / after a flagged position from the parity of every polygon's
//                      rank at that position (binary searches in the sorted keys); the flag stays iff the union changes there and no
//                      earlier polygon of the object changes at the same position; scan -> rank
//   pr_write_kernel    output index = the object's first rank + the flagged keys of the object's polygons below the position
//   pr_offsets_kernel  trans_off[o] = rank at the first point of object o
// A sorted key array and integer ranks make the result a function of the input alone: bit-identical whatever the grouping.
#include "common.h"
#include "upsnet_hip.h"

#define PR_BT 256
#define PR_ITEMS 16                       // scan: items per thread
#define PR_TILE (PR_BT * PR_ITEMS)        // scan: items per workgroup
#define PR_CH 4096                        // sort: keys per LDS run (32 KiB)
#define PR_ST 512                         // sort: threads per workgroup
#define PR_NONE 0x7FFFFFFFu               // position of a point that emits nothing (>= h * w, sorts last in its polygon)
#define PR_MAX_POINTS (1L << 24)

typedef unsigned long long pr_u64;

// ------------------------------------------------------------------------------------------------------------------ helpers
// the number of entries of a[0 .. n) that are <= v (a ascending)
__device__ static inline int pr_upper_i(const int *__restrict__ a, const int n, const int v)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int m = (lo + hi) >> 1; if (a[m] <= v) lo = m + 1; else hi = m; }
    return lo;
}

// the first index in [lo, hi) whose key is >= k (keys ascending there)
__device__ static inline int pr_lower_k(const pr_u64 *__restrict__ keys, int lo, int hi, const pr_u64 k)
{
    while (lo < hi) { const int m = (lo + hi) >> 1; if (keys[m] < k) lo = m + 1; else hi = m; }
    return lo;
}

// first point of vertex / edge v, never beyond the N points the workspace holds
__device__ static inline int pr_first(const int *__restrict__ eoff, const int v, const int N) { return min(eoff[v], N); }

// point d (0 .. count - 1, in edge direction) of the edge (xs, ys) -> (xe, ye): rleFrPoly's upsampled walk
__device__ static inline void pr_point(int xs, int ys, int xe, int ye, const int d, int *u, int *v)
{
    const int dx = abs(xe - xs), dy = abs(ys - ye);
    const bool flip = (dx >= dy && xs > xe) || (dx < dy && ys > ye);
    if (flip) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    if (dx >= dy) {
        const int t = flip ? dx - d : d;
        *u = t + xs;
        *v = dx == 0 ? ys : (int)((double)ys + ((double)(ye - ys) / (double)dx) * (double)t + .5);
    } else {
        const int t = flip ? dy - d : d;
        *v = t + ys;
        *u = (int)((double)xs + ((double)(xe - xs) / (double)dy) * (double)t + .5);
    }
}

// ------------------------------------------------------------------------------------------------------------------ scan
// exclusive prefix sums of in[0 .. n) into out[0 .. n], out[n] = the total (32-bit: the caller bounds the total)
__device__ static inline int pr_block_exclusive(const int v, int *s, int *total)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int o = 1; o < PR_BT; o <<= 1) {
        const int a = tid >= o ? s[tid - o] : 0;
        __syncthreads();
        s[tid] += a;
        __syncthreads();
    }
    const int incl = s[tid];
    *total = s[PR_BT - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(PR_BT)
pr_scan_reduce_kernel(const int *__restrict__ in, const int n, int *__restrict__ part)
{
    __shared__ int s[PR_BT];
    const long base = (long)blockIdx.x * PR_TILE + (long)threadIdx.x * PR_ITEMS;
    int sum = 0;
    for (int k = 0; k < PR_ITEMS; ++k) sum += base + k < n ? in[base + k] : 0;
    int total;
    pr_block_exclusive(sum, s, &total);
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ void __launch_bounds__(PR_BT)
pr_scan_parts_kernel(int *__restrict__ part, const int nb)
{
    __shared__ int s[PR_BT];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += PR_BT) {
        const int i = b0 + threadIdx.x;
        const int v = i < nb ? part[i] : 0;
        int total;
        const int ex = pr_block_exclusive(v, s, &total);
        if (i < nb) part[i] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(PR_BT)
pr_scan_apply_kernel(const int *__restrict__ in, const int n, const int *__restrict__ part, int *__restrict__ out)
{
    __shared__ int s[PR_BT];
    const long base = (long)blockIdx.x * PR_TILE + (long)threadIdx.x * PR_ITEMS;
    int v[PR_ITEMS];
    int sum = 0;
    for (int k = 0; k < PR_ITEMS; ++k) { v[k] = base + k < n ? in[base + k] : 0; sum += v[k]; }
    int total;
    int run = part[blockIdx.x] + pr_block_exclusive(sum, s, &total);
    for (int k = 0; k < PR_ITEMS; ++k) {
        if (base + k <= n) out[base + k] = run;   // index n takes the grand total
        run += v[k];
    }
}

// ------------------------------------------------------------------------------------------------------------------ edges, points
__global__ void __launch_bounds__(PR_BT)
pr_vertex_kernel(const double *__restrict__ verts, const int *__restrict__ poly_off, const int P, const int TV, int2 *__restrict__ xy,
                 int *__restrict__ cnt)
{
    const int v = blockIdx.x * PR_BT + threadIdx.x;
    if (v >= TV) return;
    const int q = pr_upper_i(poly_off, P + 1, v) - 1;
    const int nx = v + 1 < poly_off[q + 1] ? v + 1 : poly_off[q];
    const int X = (int)(5 * verts[2 * (long)v] + .5), Y = (int)(5 * verts[2 * (long)v + 1] + .5);
    const int Xn = (int)(5 * verts[2 * (long)nx] + .5), Yn = (int)(5 * verts[2 * (long)nx + 1] + .5);
    xy[v] = make_int2(X, Y);
    const long d = max(labs((long)Xn - X), labs((long)Yn - Y)) + 1;
    cnt[v] = (int)min(d, PR_MAX_POINTS + 1);   // the host refuses such input; the clamp keeps the 32-bit prefix from wrapping
}

// keys[i], i < M: point i's (polygon << 32 | position), PR_NONE as the position of a point that emits none; ~0 for i >= the points
__global__ void __launch_bounds__(PR_BT)
pr_emit_kernel(const int2 *__restrict__ xy, const int *__restrict__ eoff, const int *__restrict__ poly_off, const int P, const int TV,
               const int N, const int M, const int H, const int W, pr_u64 *__restrict__ keys)
{
    const int i = blockIdx.x * PR_BT + threadIdx.x;
    if (i >= M) return;
    if (i >= pr_first(eoff, TV, N)) { keys[i] = ~0ull; return; }
    const int e = pr_upper_i(eoff, TV + 1, i) - 1;       // the edge of point i (every edge has at least one point)
    const int q = pr_upper_i(poly_off, P + 1, e) - 1;
    const int v0 = poly_off[q], v1 = poly_off[q + 1];
    pr_u64 key = ((pr_u64)(unsigned)q << 32) | PR_NONE;
    if (i > eoff[v0]) {   // a polygon's first point has no predecessor
        const int d = i - eoff[e];
        const int2 a = xy[e], b = xy[e + 1 < v1 ? e + 1 : v0];
        int u, v, up, vp;
        pr_point(a.x, a.y, b.x, b.y, d, &u, &v);
        if (d > 0) pr_point(a.x, a.y, b.x, b.y, d - 1, &up, &vp);
        else {
            const int2 c = xy[e - 1];
            pr_point(c.x, c.y, a.x, a.y, eoff[e] - eoff[e - 1] - 1, &up, &vp);
        }
        if (u != up) {
            double xd = (double)(u < up ? u : u - 1);
            xd = (xd + .5) / 5 - .5;
            if (floor(xd) == xd && xd >= 0 && xd <= (double)(W - 1)) {
                double yd = (double)(v < vp ? v : vp);
                yd = (yd + .5) / 5 - .5;
                if (yd < 0) yd = 0; else if (yd > (double)H) yd = (double)H;
                yd = ceil(yd);
                const long pos = (long)(int)xd * H + (int)yd;
                if (pos < (long)H * W) key = ((pr_u64)(unsigned)q << 32) | (pr_u64)pos;
            }
        }
    }
    keys[i] = key;
}

// ------------------------------------------------------------------------------------------------------------------ sort
__device__ static inline void pr_cmpx(pr_u64 *a, pr_u64 *b, const bool asc)
{
    const pr_u64 x = *a, y = *b;
    if ((x > y) == asc) { *a = y; *b = x; }
}

// LDS part of the bitonic network over run blockIdx.x: stages k = k0 .. k1 (k doubling), each with the strides min(k / 2, PR_CH / 2)
// .. 1; the direction of a comparator comes from the global index of its lower element and the stage
__global__ void __launch_bounds__(PR_ST)
pr_sort_lds_kernel(pr_u64 *__restrict__ keys, const int k0, const int k1)
{
    __shared__ pr_u64 s[PR_CH];
    const int base = blockIdx.x * PR_CH;
    for (int i = threadIdx.x; i < PR_CH; i += PR_ST) s[i] = keys[base + i];
    __syncthreads();
    for (long k = k0; k <= k1; k <<= 1) {
        for (int j = (int)min(k >> 1, (long)(PR_CH >> 1)); j > 0; j >>= 1) {
            for (int c = threadIdx.x; c < PR_CH / 2; c += PR_ST) {
                const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1));
                pr_cmpx(&s[lo], &s[lo | j], (((long)(base + lo)) & k) == 0);
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < PR_CH; i += PR_ST) keys[base + i] = s[i];
}

// one compare-exchange step of stage k with stride j >= PR_CH in global memory; one thread per comparator
__global__ void __launch_bounds__(PR_BT)
pr_sort_step_kernel(pr_u64 *__restrict__ keys, const int half, const long k, const int j)
{
    const int c = blockIdx.x * PR_BT + threadIdx.x;
    if (c >= half) return;
    const int lo = ((c & ~(j - 1)) << 1) | (c & (j - 1));
    pr_cmpx(&keys[lo], &keys[lo | j], ((long)lo & k) == 0);
}

// ------------------------------------------------------------------------------------------------------------------ parity, union
__global__ void __launch_bounds__(PR_BT)
pr_parity_kernel(const pr_u64 *__restrict__ keys, const int *__restrict__ eoff, const int TV, const int N, int *__restrict__ flag)
{
    const int i = blockIdx.x * PR_BT + threadIdx.x;
    if (i >= N) return;
    const int n = pr_first(eoff, TV, N);
    int f = 0;
    if (i < n) {
        const pr_u64 k = keys[i];
        if ((unsigned)k != PR_NONE && (i == 0 || keys[i - 1] != k)) {
            int j = i + 1;
            while (j < n && keys[j] == k) ++j;
            f = (j - i) & 1;
        }
    }
    flag[i] = f;
}

struct PrObj { int q0, q1; };

__device__ static inline PrObj pr_object_of(const int *__restrict__ obj_off, const int O, const int q)
{
    const int o = pr_upper_i(obj_off, O + 1, q) - 1;
    PrObj r = {obj_off[o], obj_off[o + 1]};
    return r;
}

// flag[i] &= the union of the object's polygons changes at this position and polygon q is the first of them that changes there
__global__ void __launch_bounds__(PR_BT)
pr_union_kernel(const pr_u64 *__restrict__ keys, const int *__restrict__ eoff, const int *__restrict__ poly_off,
                const int *__restrict__ obj_off, const int O, const int N, const int *__restrict__ rank, int *__restrict__ flag)
{
    const int i = blockIdx.x * PR_BT + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const pr_u64 key = keys[i];
    const int q = (int)(key >> 32);
    const unsigned a = (unsigned)key;
    const PrObj ob = pr_object_of(obj_off, O, q);
    if (ob.q1 - ob.q0 == 1) return;
    int before = 0, after = 0, earlier = 0;
    for (int p = ob.q0; p < ob.q1; ++p) {
        const int s0 = pr_first(eoff, poly_off[p], N), s1 = pr_first(eoff, poly_off[p + 1], N);
        const pr_u64 kp = ((pr_u64)(unsigned)p << 32) | a;
        const int lb = pr_lower_k(keys, s0, s1, kp), ub = pr_lower_k(keys, lb, s1, kp + 1);
        const int below = (rank[lb] - rank[s0]) & 1, upto = (rank[ub] - rank[s0]) & 1;
        before |= below;
        after |= upto;
        if (p < q && below != upto) earlier = 1;
    }
    if (before == after || earlier) flag[i] = 0;
}

__global__ void __launch_bounds__(PR_BT)
pr_write_kernel(const pr_u64 *__restrict__ keys, const int *__restrict__ eoff, const int *__restrict__ poly_off,
                const int *__restrict__ obj_off, const int O, const int N, const int *__restrict__ flag, const int *__restrict__ rank,
                int *__restrict__ trans)
{
    const int i = blockIdx.x * PR_BT + threadIdx.x;
    if (i >= N || !flag[i]) return;
    const pr_u64 key = keys[i];
    const int q = (int)(key >> 32);
    const unsigned a = (unsigned)key;
    const PrObj ob = pr_object_of(obj_off, O, q);
    int at = rank[i];   // one polygon: the flagged keys before this one, all objects before included
    if (ob.q1 - ob.q0 > 1) {
        at = rank[pr_first(eoff, poly_off[ob.q0], N)];
        for (int p = ob.q0; p < ob.q1; ++p) {
            const int s0 = pr_first(eoff, poly_off[p], N), s1 = pr_first(eoff, poly_off[p + 1], N);
            at += rank[pr_lower_k(keys, s0, s1, ((pr_u64)(unsigned)p << 32) | a)] - rank[s0];
        }
    }
    trans[at] = (int)a;
}

// rank == null: no point at all, every list is empty
__global__ void __launch_bounds__(PR_BT)
pr_offsets_kernel(const int *__restrict__ eoff, const int *__restrict__ poly_off, const int *__restrict__ obj_off, const int O,
                  const int N, const int *__restrict__ rank, int64_t *__restrict__ trans_off)
{
    const int o = blockIdx.x * PR_BT + threadIdx.x;
    if (o > O) return;
    trans_off[o] = rank ? (int64_t)rank[pr_first(eoff, poly_off[obj_off[o]], N)] : 0;
}

// ------------------------------------------------------------------------------------------------------------------ C ABI
static inline size_t pr_align(size_t n) { return (n + 255) & ~(size_t)255; }

static inline long pr_pow2(long n)
{
    long m = PR_CH;
    while (m < n) m <<= 1;
    return m;
}

struct PrLayout {
    int2 *xy;
    int *cnt, *eoff, *part, *flag, *rank;
    pr_u64 *keys;
};

static PrLayout pr_layout(void *ws, long TV, long N, size_t *bytes)
{
    PrLayout L;
    size_t o = 0;
    const auto at = [ws](size_t off) { return ws ? (char *)ws + off : nullptr; };   // (a size-only call passes no workspace)
    const long big = TV > N ? TV : N;
    L.xy = (int2 *)at(o); o += pr_align(sizeof(int2) * TV);
    L.cnt = (int *)at(o); o += pr_align(sizeof(int) * TV);
    L.eoff = (int *)at(o); o += pr_align(sizeof(int) * (TV + 1));
    L.part = (int *)at(o); o += pr_align(sizeof(int) * ((big + PR_TILE) / PR_TILE + 1));
    L.flag = (int *)at(o); o += pr_align(sizeof(int) * N);
    L.rank = (int *)at(o); o += pr_align(sizeof(int) * (N + 1));
    L.keys = (pr_u64 *)at(o); o += pr_align(sizeof(pr_u64) * pr_pow2(N));
    if (bytes) *bytes = o;
    return L;
}

extern "C" size_t upsnet_poly_raster_workspace_bytes(long total_vertices, long total_points)
{
    if (total_vertices < 0 || total_points < 0 || total_points > PR_MAX_POINTS || total_vertices > total_points) return 0;
    size_t b = 0;
    pr_layout(nullptr, total_vertices, total_points, &b);
    return b;
}

static int pr_scan(hipStream_t st, const int *in, int n, int *part, int *out)
{
    const int nb = n / PR_TILE + 1;   // covers index n, which takes the total
    hipLaunchKernelGGL(pr_scan_reduce_kernel, dim3(nb), dim3(PR_BT), 0, st, in, n, part);
    UPS_CHECK_LAUNCH("pr_scan_reduce_kernel");
    hipLaunchKernelGGL(pr_scan_parts_kernel, dim3(1), dim3(PR_BT), 0, st, part, nb);
    UPS_CHECK_LAUNCH("pr_scan_parts_kernel");
    hipLaunchKernelGGL(pr_scan_apply_kernel, dim3(nb), dim3(PR_BT), 0, st, in, n, part, out);
    UPS_CHECK_LAUNCH("pr_scan_apply_kernel");
    return 0;
}

extern "C" int upsnet_poly_raster(void *stream, const double *vertices, const int *poly_off, const int *obj_off, const int *poly_off_dev,
                                  const int *obj_off_dev, int num_poly, int num_obj, long total_points, int height, int width,
                                  void *workspace, int *trans, int64_t *trans_off)
{
    hipStream_t st = (hipStream_t)stream;
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "poly_raster: bad image size %dx%d", height, width);
    UPS_REQUIRE(num_poly >= 0 && num_obj >= 0, "poly_raster: negative counts (%d polygons, %d objects)", num_poly, num_obj);
    UPS_REQUIRE(poly_off && obj_off && poly_off_dev && obj_off_dev && trans_off, "poly_raster: null pointer");
    UPS_REQUIRE(poly_off[0] == 0 && obj_off[0] == 0 && obj_off[num_obj] == num_poly, "poly_raster: offsets must start at 0 and the objects must "
                "cover the %d polygons", num_poly);
    for (int q = 0; q < num_poly; ++q) UPS_REQUIRE(poly_off[q + 1] >= poly_off[q], "poly_raster: poly_off decreases at polygon %d", q);
    for (int o = 0; o < num_obj; ++o) UPS_REQUIRE(obj_off[o + 1] >= obj_off[o], "poly_raster: obj_off decreases at object %d", o);
    const int TV = poly_off[num_poly], P = num_poly, O = num_obj, H = height, W = width;
    UPS_REQUIRE(total_points >= TV && total_points <= PR_MAX_POINTS, "poly_raster: %ld points for %d vertices (every vertex starts an edge of "
                "at least one point; at most %ld points a call)", total_points, TV, PR_MAX_POINTS);
    const int N = (int)total_points;
    if (TV == 0) {   // no vertex, no point: every list is empty
        hipLaunchKernelGGL(pr_offsets_kernel, dim3(ups_divup(O + 1, PR_BT)), dim3(PR_BT), 0, st, (const int *)nullptr, poly_off_dev,
                           obj_off_dev, O, 0, (const int *)nullptr, trans_off);
        UPS_CHECK_LAUNCH("pr_offsets_kernel");
        return 0;
    }
    UPS_REQUIRE(vertices && workspace && trans, "poly_raster: null pointer");
    const PrLayout L = pr_layout(workspace, TV, N, nullptr);
    const int M = (int)pr_pow2(N);
    hipLaunchKernelGGL(pr_vertex_kernel, dim3(ups_divup(TV, PR_BT)), dim3(PR_BT), 0, st, vertices, poly_off_dev, P, TV, L.xy, L.cnt);
    UPS_CHECK_LAUNCH("pr_vertex_kernel");
    if (pr_scan(st, L.cnt, TV, L.part, L.eoff)) return 1;
    hipLaunchKernelGGL(pr_emit_kernel, dim3(ups_divup(M, PR_BT)), dim3(PR_BT), 0, st, L.xy, L.eoff, poly_off_dev, P, TV, N, M, H, W, L.keys);
    UPS_CHECK_LAUNCH("pr_emit_kernel");
    hipLaunchKernelGGL(pr_sort_lds_kernel, dim3(M / PR_CH), dim3(PR_ST), 0, st, L.keys, 2, PR_CH);
    UPS_CHECK_LAUNCH("pr_sort_lds_kernel");
    for (long k = 2L * PR_CH; k <= M; k <<= 1) {
        for (long j = k >> 1; j >= PR_CH; j >>= 1) {
            hipLaunchKernelGGL(pr_sort_step_kernel, dim3(ups_divup(M / 2, PR_BT)), dim3(PR_BT), 0, st, L.keys, M / 2, k, (int)j);
            UPS_CHECK_LAUNCH("pr_sort_step_kernel");
        }
        hipLaunchKernelGGL(pr_sort_lds_kernel, dim3(M / PR_CH), dim3(PR_ST), 0, st, L.keys, (int)k, (int)k);
        UPS_CHECK_LAUNCH("pr_sort_lds_kernel");
    }
    const dim3 gn(ups_divup(N, PR_BT));
    hipLaunchKernelGGL(pr_parity_kernel, gn, dim3(PR_BT), 0, st, L.keys, L.eoff, TV, N, L.flag);
    UPS_CHECK_LAUNCH("pr_parity_kernel");
    if (pr_scan(st, L.flag, N, L.part, L.rank)) return 1;
    hipLaunchKernelGGL(pr_union_kernel, gn, dim3(PR_BT), 0, st, L.keys, L.eoff, poly_off_dev, obj_off_dev, O, N, L.rank, L.flag);
    UPS_CHECK_LAUNCH("pr_union_kernel");
    if (pr_scan(st, L.flag, N, L.part, L.rank)) return 1;
    hipLaunchKernelGGL(pr_write_kernel, gn, dim3(PR_BT), 0, st, L.keys, L.eoff, poly_off_dev, obj_off_dev, O, N, L.flag, L.rank, trans);
    UPS_CHECK_LAUNCH("pr_write_kernel");
    hipLaunchKernelGGL(pr_offsets_kernel, dim3(ups_divup(O + 1, PR_BT)), dim3(PR_BT), 0, st, L.eoff, poly_off_dev, obj_off_dev, O, N, L.rank,
                       trans_off);
    UPS_CHECK_LAUNCH("pr_offsets_kernel");
    return 0;
}
