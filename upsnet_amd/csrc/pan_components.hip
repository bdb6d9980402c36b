// pan_components.hip -- connected components of a 2-channel panoptic map and the removal of small fragments (gfx950), DESIGN.md 4.26.
//
// The reference has no connected-component step: the rule is this project's own, stated in include/upsnet_hip.h and restated in plain
// numpy (and once more on scipy.ndimage.label) in tests/pan_components_ref.py. Integers throughout.
//
// A pixel's key is c << 8 | i (bytes 0 and 1; byte 2 is never read); c == 255 is VOID and belongs to no component. A component is a
// maximal set of pixels of one key connected under 4- or 8-connectivity; its label is the smallest linear index y * W + x among its
// pixels, so nothing depends on the order of execution. Labels are kept as a union-find forest over the pixels, parent[p] <= p, a root
// has parent[p] == p, VOID has -1.
//
// Five launches, no host read between them; the workspace may hold anything on entry:
//   pc_tile_kernel     one workgroup per 32 x 128 tile, 16 pixels of one row per thread (pan_pixels.h's loads). LDS holds the tile's keys
//                      and labels. A pixel is seeded with the head of its run inside the thread's 16 pixels; then unions with the
//                      neighbouring thread's last pixel and with the row above (for 8-connectivity the two upper diagonals, only where
//                      the pixel above has another key: where it has the same one, the row above links its neighbours already) by
//                      union-find with LDS atomicMin; then every pixel stores the global index of its local root. The kernel also
//                      zeroes area[], best[] and stats[].
//   pc_seam_kernel     one thread per pixel of the first row of every tile row but the first and of the first column of every tile
//                      column but the first: the same unions across the seam, in global memory.
//   pc_flatten_kernel  parent[p] = find(p); area[root] += with one atomic per run of equal root inside a thread's 16 pixels.
//   pc_main_kernel     root pixels only: atomicMax of area << 32 | (0xffffffff - p) into best[key] -- the largest area, ties to the
//                      smaller label; the first arrival at a key counts it; every root counts a component.
//   pc_apply_kernel    writes the output map (removed components become (255, 0, byte 2)), the optional label map and the removal
//                      counts, wave-reduced.
#include "common.h"
#include "upsnet_hip.h"
#include "pan_pixels.h"

#define PC_KEYS 65536
#define PC_TH 32                  // tile height
#define PC_TW 128                 // tile width
#define PC_T 256                  // threads per workgroup: PC_TH rows x PC_TW / PAN_RUN threads of 16 pixels
#define PC_VOID 0xffffu
#define PC_MAX_PIXELS (1L << 24)

// Workspace: best[PC_KEYS] (uint64) | parent[npix] (int) | area[npix] (int)
struct PcWs {
    unsigned long long *best;
    int *parent, *area;
};

static PcWs pc_ws(void *base, const long npix)
{
    PcWs w;
    w.best = (unsigned long long *)base;
    w.parent = (int *)(w.best + PC_KEYS);
    w.area = w.parent + ((npix + 3) & ~3L);      // (keeps area[] 16-byte aligned)
    return w;
}

__device__ static inline unsigned pc_key_of(const unsigned c, const unsigned i) { return c == 255 ? PC_VOID : (c << 8 | i); }

// n (0..16) ints from src + p0: four 16-byte accesses when whole and p0 is a multiple of 4 (src is 16-byte aligned), else one by one
__device__ static inline void pc_load_ints(const int *src, const long p0, const int n, int v[PAN_RUN])
{
    if (n == PAN_RUN && (p0 & 3) == 0) {
        const int4 *q = (const int4 *)(src + p0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int4 a = q[j];
            v[4 * j] = a.x; v[4 * j + 1] = a.y; v[4 * j + 2] = a.z; v[4 * j + 3] = a.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) v[j] = j < n ? src[p0 + j] : -1;
    }
}

__device__ static inline void pc_store_ints(int *dst, const long p0, const int n, const int v[PAN_RUN])
{
    if (n == PAN_RUN && (p0 & 3) == 0) {
        int4 *q = (int4 *)(dst + p0);
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = make_int4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j)
            if (j < n) dst[p0 + j] = v[j];
    }
}

__device__ static inline int pc_wave_sum(int v)
{
#pragma unroll
    for (int o = UPS_WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- tile pass (LDS)
__device__ static inline int pc_find_lds(int *lab, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(&lab[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == x) return x;
        x = p;
    }
}

// Labels only ever decrease and lab[x] <= x. atomicMin on the larger root's cell: if the old value is that root, it was a root and now
// hangs under the smaller one; otherwise somebody else moved it in between, and the union goes on between the old value and the smaller
// root (the cell may now point at either: both are in the component being formed).
__device__ static inline void pc_union_lds(int *lab, int a, int b)
{
    for (;;) {
        a = pc_find_lds(lab, a);
        b = pc_find_lds(lab, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(&lab[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ void __launch_bounds__(PC_T)
pc_tile_kernel(const unsigned char *__restrict__ pan, const int H, const int W, const int tiles_x, const int conn8, const bool vec,
               PcWs ws, int *__restrict__ stats)
{
    __shared__ unsigned short s_key[PC_TH * PC_TW];
    __shared__ int s_lab[PC_TH * PC_TW];
    const int t = threadIdx.x;
    for (unsigned i = blockIdx.x * PC_T + t; i < PC_KEYS; i += gridDim.x * PC_T) ws.best[i] = 0ull;
    if (blockIdx.x == 0 && t < 4) stats[t] = 0;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int ly = t / (PC_TW / PAN_RUN), lx0 = (t % (PC_TW / PAN_RUN)) * PAN_RUN;
    const int gy = ty * PC_TH + ly, gx0 = tx * PC_TW + lx0;
    const int n = gy < H ? max(0, min(PAN_RUN, W - gx0)) : 0;      // pixels of this thread inside the image
    const long gp = (long)gy * W + gx0;
    const long q0 = n ? gp : 0;                                   // (a thread outside the image reads and writes nothing)
    unsigned w[12];
    pan_load48(pan, q0, q0 + n, vec, w);
    unsigned k[PAN_RUN];
    const int base = ly * PC_TW + lx0;
    int head = base;
#pragma unroll
    for (int j = 0; j < PAN_RUN; ++j) {
        k[j] = j < n ? pc_key_of(pan_byte(w, 3 * j), pan_byte(w, 3 * j + 1)) : PC_VOID;
        if (j > 0 && k[j] != k[j - 1]) head = base + j;
        s_key[base + j] = (unsigned short)k[j];
        s_lab[base + j] = head;
    }
    {
        int z[PAN_RUN];
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) z[j] = 0;
        pc_store_ints(ws.area, q0, n, z);
    }
    __syncthreads();
    if (lx0 > 0 && k[0] != PC_VOID && s_key[base - 1] == k[0]) pc_union_lds(s_lab, base, base - 1);
    if (ly > 0) {
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) {
            const unsigned kj = k[j];
            if (kj == PC_VOID) continue;
            const int q = base + j, lx = lx0 + j;
            if (s_key[q - PC_TW] == kj) {
                // (inside a run that continues above as one run, the run's first pixel has made the link)
                if (j == 0 || k[j - 1] != kj || s_key[q - PC_TW - 1] != kj) pc_union_lds(s_lab, q, q - PC_TW);
            } else if (conn8) {
                if (lx > 0 && s_key[q - PC_TW - 1] == kj) pc_union_lds(s_lab, q, q - PC_TW - 1);
                if (lx < PC_TW - 1 && s_key[q - PC_TW + 1] == kj) pc_union_lds(s_lab, q, q - PC_TW + 1);
            }
        }
    }
    __syncthreads();
    int out[PAN_RUN];
    int root = 0;
#pragma unroll
    for (int j = 0; j < PAN_RUN; ++j) {
        if (k[j] == PC_VOID) {
            out[j] = -1;
        } else {
            if (j == 0 || k[j] != k[j - 1]) {     // (equal neighbours in a row share their root)
                const int r = pc_find_lds(s_lab, base + j);
                root = (ty * PC_TH + r / PC_TW) * W + tx * PC_TW + r % PC_TW;
            }
            out[j] = root;
        }
    }
    pc_store_ints(ws.parent, q0, n, out);
}

// ---------------------------------------------------------------------------------------------------------------- global union-find
// Every access to parent[] inside a launch that changes it is an agent-scope atomic: the loads bypass the CU's L1, which no other CU's
// store refreshes. Even a stale value would only cost an iteration: every value a cell has held is an ancestor-to-be of the pixel (a
// thread that replaces a non-root cell's value goes on to unite the old value with the new one), and the value atomicMin returns, the
// only one a decision rests on, is the cell's true one.
__device__ static inline int pc_find(int *parent, int x)
{
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == x) return x;
        x = p;
    }
}

__device__ static inline void pc_union(int *parent, int a, int b)
{
    for (;;) {
        a = pc_find(parent, a);
        b = pc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int s = a; a = b; b = s; }
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

__device__ static inline unsigned pc_key_at(const unsigned char *__restrict__ pan, const long p)
{
    return pc_key_of(pan[3 * p], pan[3 * p + 1]);
}

__global__ void __launch_bounds__(PC_T)
pc_seam_kernel(const unsigned char *__restrict__ pan, const int H, const int W, const long nh, const long nv, const int conn8, int *parent)
{
    long idx = (long)blockIdx.x * PC_T + threadIdx.x;
    if (idx < nh) {
        // first row of a tile row against the row above
        const int y = (int)(idx / W + 1) * PC_TH, x = (int)(idx % W);
        const long p = (long)y * W + x;
        const unsigned k = pc_key_at(pan, p);
        if (k == PC_VOID) return;
        if (pc_key_at(pan, p - W) == k) {
            pc_union(parent, (int)p, (int)(p - W));
        } else if (conn8) {
            if (x > 0 && pc_key_at(pan, p - W - 1) == k) pc_union(parent, (int)p, (int)(p - W - 1));
            if (x < W - 1 && pc_key_at(pan, p - W + 1) == k) pc_union(parent, (int)p, (int)(p - W + 1));
        }
    } else if (idx < nh + nv) {
        // first column of a tile column against the column to its left
        idx -= nh;
        const int x = (int)(idx / H + 1) * PC_TW, y = (int)(idx % H);
        const long p = (long)y * W + x;
        const unsigned k = pc_key_at(pan, p);
        if (k == PC_VOID) return;
        if (pc_key_at(pan, p - 1) == k) {
            pc_union(parent, (int)p, (int)(p - 1));
        } else if (conn8) {
            if (y > 0 && pc_key_at(pan, p - W - 1) == k) pc_union(parent, (int)p, (int)(p - W - 1));
            if (y < H - 1 && pc_key_at(pan, p + W - 1) == k) pc_union(parent, (int)p, (int)(p + W - 1));
        }
    }
}

// No union runs in this launch: a cell holds its parent of the seam pass or, once a thread has flattened it, its root; find() ends at
// the same root through either.
__global__ void __launch_bounds__(PC_T)
pc_flatten_kernel(const long npix, PcWs ws)
{
    const long p0 = ((long)blockIdx.x * PC_T + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    const int n = (int)min((long)PAN_RUN, npix - p0);
    int v[PAN_RUN];
    pc_load_ints(ws.parent, p0, n, v);
    int prev = -1, root = -1, run_root = -1, run = 0;
#pragma unroll
    for (int j = 0; j < PAN_RUN; ++j) {
        if (j < n && v[j] >= 0) {
            if (v[j] != prev) {
                prev = v[j];
                root = pc_find(ws.parent, prev);
            }
            v[j] = root;
            if (root != run_root) {
                if (run) atomicAdd(&ws.area[run_root], run);
                run_root = root;
                run = 0;
            }
            ++run;
        }
    }
    if (run) atomicAdd(&ws.area[run_root], run);
    pc_store_ints(ws.parent, p0, n, v);
}

__global__ void __launch_bounds__(PC_T)
pc_main_kernel(const unsigned char *__restrict__ pan, const long npix, PcWs ws, int *stats)
{
    const long p0 = ((long)blockIdx.x * PC_T + threadIdx.x) * PAN_RUN;
    int ncomp = 0, nkeys = 0;
    if (p0 < npix) {
        const int n = (int)min((long)PAN_RUN, npix - p0);
        int v[PAN_RUN];
        pc_load_ints(ws.parent, p0, n, v);
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) {
            if (j < n && v[j] == (int)(p0 + j)) {
                const unsigned p = (unsigned)(p0 + j);
                const unsigned long long cand = (unsigned long long)(unsigned)ws.area[p] << 32 | (0xffffffffu - p);
                const unsigned long long old = atomicMax(&ws.best[pc_key_at(pan, p)], cand);
                ++ncomp;
                nkeys += old == 0ull;             // (an area is >= 1: no candidate is 0)
            }
        }
    }
    ncomp = pc_wave_sum(ncomp);
    nkeys = pc_wave_sum(nkeys);
    if ((threadIdx.x & (UPS_WAVE - 1)) == 0) {
        if (nkeys) atomicAdd(&stats[0], nkeys);
        if (ncomp) atomicAdd(&stats[1], ncomp);
    }
}

// pan and out may be one buffer: a thread reads its own 16 pixels before it writes them, and nobody else touches them
__global__ void __launch_bounds__(PC_T)
pc_apply_kernel(const unsigned char *pan, unsigned char *out, int *labels, const long npix, const bool vec, const int min_area,
                const int keep_largest, PcWs ws, int *stats)
{
    const long p0 = ((long)blockIdx.x * PC_T + threadIdx.x) * PAN_RUN;
    int ncomp = 0, npixels = 0;
    if (p0 < npix) {
        const int n = (int)min((long)PAN_RUN, npix - p0);
        unsigned w[12];
        int v[PAN_RUN];
        pan_load48(pan, p0, p0 + n, vec, w);
        pc_load_ints(ws.parent, p0, n, v);
        int prev = -1;
        bool removed = false;
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) {
            if (j < n && v[j] >= 0) {
                if (v[j] != prev) {
                    prev = v[j];
                    removed = ws.area[prev] < min_area;
                    if (removed && keep_largest) {
                        const unsigned key = pan_byte(w, 3 * j) << 8 | pan_byte(w, 3 * j + 1);
                        removed = (unsigned)ws.best[key] != 0xffffffffu - (unsigned)prev;
                    }
                }
                if (removed) {
                    w[(3 * j) >> 2] |= 255u << (8 * ((3 * j) & 3));                 // category 255
                    w[(3 * j + 1) >> 2] &= ~(255u << (8 * ((3 * j + 1) & 3)));      // instance 0; byte 2 stays
                    ++npixels;
                    ncomp += prev == (int)(p0 + j);
                }
            }
        }
        pan_store48(out, p0, p0 + n, vec, w);
        if (labels) pc_store_ints(labels, p0, n, v);
    }
    ncomp = pc_wave_sum(ncomp);
    npixels = pc_wave_sum(npixels);
    if ((threadIdx.x & (UPS_WAVE - 1)) == 0 && npixels) {
        if (ncomp) atomicAdd(&stats[2], ncomp);
        atomicAdd(&stats[3], npixels);
    }
}

extern "C" size_t upsnet_pan_components_workspace_bytes(int height, int width)
{
    if (height < 1 || width < 1 || (long)height * width > PC_MAX_PIXELS) return 0;
    const long npix = (long)height * width;
    return (size_t)PC_KEYS * sizeof(unsigned long long) + (size_t)(((npix + 3) & ~3L) + npix) * sizeof(int);
}

extern "C" int upsnet_pan_components(void *stream, const unsigned char *pan_2ch, int height, int width, int connectivity, int min_area,
                                     int keep_largest, void *workspace, unsigned char *out_2ch, int *labels, int *stats)
{
    UPS_REQUIRE(pan_2ch && workspace && out_2ch && stats, "pan_components: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= PC_MAX_PIXELS, "pan_components: image of %d x %d pixels outside 1..2^24",
                height, width);
    UPS_REQUIRE(connectivity == 4 || connectivity == 8, "pan_components: connectivity %d is neither 4 nor 8", connectivity);
    UPS_REQUIRE(min_area >= 0, "pan_components: min_area %d is negative", min_area);
    UPS_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)labels & 15) == 0 && ((uintptr_t)stats & 3) == 0,
                "pan_components: workspace / labels not 16-byte aligned, or stats not 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)height * width;
    PcWs ws = pc_ws(workspace, npix);
    const int tiles_x = ups_divup(width, PC_TW), tiles_y = ups_divup(height, PC_TH);
    const int conn8 = connectivity == 8;
    const bool vec_in = ((uintptr_t)pan_2ch & 15) == 0;
    // (a thread's 16 pixels of a tile row start at y * W + a multiple of 16: 16-byte loads need W % 16 == 0 as well)
    hipLaunchKernelGGL(pc_tile_kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(PC_T), 0, st, pan_2ch, height, width, tiles_x, conn8,
                       vec_in && (width & 15) == 0, ws, stats);
    UPS_CHECK_LAUNCH("pc_tile_kernel");
    const long nh = (long)(tiles_y - 1) * width, nv = (long)(tiles_x - 1) * height;
    if (nh + nv > 0) {
        hipLaunchKernelGGL(pc_seam_kernel, dim3((unsigned)((nh + nv + PC_T - 1) / PC_T)), dim3(PC_T), 0, st, pan_2ch, height, width, nh, nv,
                           conn8, ws.parent);
        UPS_CHECK_LAUNCH("pc_seam_kernel");
    }
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const unsigned grid = (unsigned)((threads + PC_T - 1) / PC_T);
    hipLaunchKernelGGL(pc_flatten_kernel, dim3(grid), dim3(PC_T), 0, st, npix, ws);
    UPS_CHECK_LAUNCH("pc_flatten_kernel");
    hipLaunchKernelGGL(pc_main_kernel, dim3(grid), dim3(PC_T), 0, st, pan_2ch, npix, ws, stats);
    UPS_CHECK_LAUNCH("pc_main_kernel");
    hipLaunchKernelGGL(pc_apply_kernel, dim3(grid), dim3(PC_T), 0, st, pan_2ch, out_2ch, labels, npix,
                       vec_in && ((uintptr_t)out_2ch & 15) == 0, min_area, keep_largest != 0, ws, stats);
    UPS_CHECK_LAUNCH("pc_apply_kernel");
    return 0;
}
