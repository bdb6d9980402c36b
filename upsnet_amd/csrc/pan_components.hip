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
// upsnet_pan_absorb runs the same four labelling launches (pc_label) and then votes, picks and applies: see "absorb"
// below.
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

// the removal rule, for a non-VOID pixel of key `key` whose component has the label `root`
__device__ static inline bool pc_removed(const PcWs &ws, const int root, const unsigned key, const int min_area, const int keep_largest)
{
    bool removed = ws.area[root] < min_area;
    if (removed && keep_largest) removed = (unsigned)ws.best[key] != 0xffffffffu - (unsigned)root;
    return removed;
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
                    removed = pc_removed(ws, prev, pan_byte(w, 3 * j) << 8 | pan_byte(w, 3 * j + 1), min_area, keep_largest);
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

// ---------------------------------------------------------------------------------------------------------------- absorb (4.27)
// upsnet_pan_absorb: a removed component (a FRAGMENT) takes the key of the kept segment it shares the longest border with. After the
// labelling launches above:
//   pa_vote_kernel   16 pixels per thread. A thread that holds fragment pixels looks at their four edge neighbours; a neighbour that is
//                    not VOID and not itself a fragment pixel (the apply pass's test on its root) gives its key one vote from the
//                    fragment. Equal (root, key) votes of consecutive pixels are merged before they go to the vote table: open
//                    addressing in global memory, a 64-bit word ((root << 16 | key) + 1, 0 = free) claimed by CAS, a 32-bit count
//                    beside it. The thread that owns a fragment's root pixel zeroes the fragment's winner cell.
//   pa_pick_kernel   over the table's slots, eight per thread: atomicMax of count << 16 | (0xffff - key) into winner[root] -- most
//                    votes, ties to the smaller key; a winner of 0 means no vote. Counts the slots in use (stats[6]).
//   pa_apply_kernel  pc_apply_kernel with the winner's key in place of VOID where there is one; its counts (stats[2..5]) are summed
//                    over the workgroup first.
// pa_clear_kernel, launched first, zeroes the table and stats[4..7].
//
// The table has 2 * H * W slots. A (fragment, key) pair needs a grid edge between a fragment pixel and a kept pixel and the grid has
// 2HW - H - W edges, so there are always fewer pairs than slots: a probe sequence that walks the whole table finds the pair's slot or a
// free one, and an insertion cannot fail. stats[7] is set should a walk ever come round (it cannot); the apply pass then copies its
// input. In a map of few fragments the table is nearly empty and a probe ends at its first slot.
#define PA_PICK 8                 // table slots per thread of the pick launch

struct PaWs {
    unsigned long long *winner, *tkey;
    unsigned *tcount;
    unsigned slots;
};

static size_t pa_pad16(const size_t n) { return (n + 15) & ~(size_t)15; }
static size_t pa_winner_offset(const long npix)
{
    return pa_pad16((size_t)PC_KEYS * sizeof(unsigned long long) + (size_t)(((npix + 3) & ~3L) + npix) * sizeof(int));
}
static size_t pa_table_bytes(const long npix) { return 16 * (size_t)npix + pa_pad16(8 * (size_t)npix); }   // tkey | tcount

// Workspace: best | parent | area as above | winner[npix] (uint64) | tkey[2 npix] (uint64) | tcount[2 npix] (uint), each 16-byte aligned
static PaWs pa_ws(void *base, const long npix)
{
    PaWs t;
    t.winner = (unsigned long long *)((char *)base + pa_winner_offset(npix));
    t.tkey = (unsigned long long *)((char *)t.winner + pa_pad16(8 * (size_t)npix));
    t.slots = (unsigned)(2 * npix);
    t.tcount = (unsigned *)(t.tkey + t.slots);
    return t;
}

__global__ void __launch_bounds__(PC_T)
pa_clear_kernel(uint4 *__restrict__ table, const long n16, int *__restrict__ stats)
{
    if (blockIdx.x == 0 && threadIdx.x < 4) stats[4 + threadIdx.x] = 0;
    for (long i = (long)blockIdx.x * PC_T + threadIdx.x; i < n16; i += (long)gridDim.x * PC_T) table[i] = make_uint4(0u, 0u, 0u, 0u);
}

// v votes of the fragment `root` for `key`. The words of the table change during this launch: they are read and written with
// agent-scope atomics only.
__device__ static inline void pa_vote(const PaWs &t, int *stats, const int root, const unsigned key, const int v)
{
    const unsigned long long want = ((unsigned long long)(unsigned)root << 16 | key) + 1;
    unsigned long long h = want * 0x9e3779b97f4a7c15ull;
    h ^= h >> 32;
    unsigned slot = (unsigned)(((h & 0xffffffffull) * t.slots) >> 32);
    for (unsigned n = 0; n < t.slots; ++n) {
        unsigned long long k = __hip_atomic_load(&t.tkey[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0ull) {
            k = atomicCAS(&t.tkey[slot], 0ull, want);
            if (k == 0ull) k = want;
        }
        if (k == want) {
            atomicAdd(&t.tcount[slot], (unsigned)v);
            return;
        }
        if (++slot == t.slots) slot = 0;
    }
    atomicExch(&stats[7], 1);
}

// votes waiting for their neighbours' equal ones
struct PaPending {
    int root, count;
    unsigned key;
};

__device__ static inline void pa_pending_add(PaPending &a, const PaWs &t, int *stats, const int root, const unsigned key)
{
    if (a.count && (a.root != root || a.key != key)) {
        pa_vote(t, stats, a.root, a.key, a.count);
        a.count = 0;
    }
    a.root = root;
    a.key = key;
    ++a.count;
}

// the key of pixel q if it is a kept pixel, else PC_VOID
__device__ static inline unsigned pa_kept_key(const unsigned char *__restrict__ pan, const PcWs &ws, const long q, const int min_area,
                                              const int keep_largest)
{
    const unsigned k = pc_key_at(pan, q);
    if (k == PC_VOID) return PC_VOID;
    return pc_removed(ws, ws.parent[q], k, min_area, keep_largest) ? PC_VOID : k;
}

__global__ void __launch_bounds__(PC_T)
pa_vote_kernel(const unsigned char *__restrict__ pan, const int H, const int W, const bool vec, const int min_area, const int keep_largest,
               PcWs ws, PaWs t, int *stats)
{
    const long npix = (long)H * W;
    const long p0 = ((long)blockIdx.x * PC_T + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    const int n = (int)min((long)PAN_RUN, npix - p0);
    unsigned w[12];
    int v[PAN_RUN];
    pan_load48(pan, p0, p0 + n, vec, w);
    pc_load_ints(ws.parent, p0, n, v);
    unsigned frag = 0;                    // bit j: pixel p0 + j belongs to a fragment
    {
        int prev = -1;
        bool removed = false;
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) {
            if (j < n && v[j] >= 0) {
                if (v[j] != prev) {
                    prev = v[j];
                    removed = pc_removed(ws, prev, pan_byte(w, 3 * j) << 8 | pan_byte(w, 3 * j + 1), min_area, keep_largest);
                }
                if (removed) {
                    frag |= 1u << j;
                    if (prev == (int)(p0 + j)) t.winner[prev] = 0ull;
                }
            }
        }
    }
    if (!frag) return;
    PaPending up = {0, 0, 0u}, down = {0, 0, 0u}, side = {0, 0, 0u};
    int x = (int)(p0 % W), y = (int)(p0 / W);
#pragma unroll
    for (int j = 0; j < PAN_RUN; ++j) {
        if (j < n) {
            if (frag >> j & 1) {
                const long p = p0 + j;
                const int root = v[j];
                if (y > 0) {
                    const unsigned k = pa_kept_key(pan, ws, p - W, min_area, keep_largest);
                    if (k != PC_VOID) pa_pending_add(up, t, stats, root, k);
                }
                if (y < H - 1) {
                    const unsigned k = pa_kept_key(pan, ws, p + W, min_area, keep_largest);
                    if (k != PC_VOID) pa_pending_add(down, t, stats, root, k);
                }
                // (a left or right neighbour among the thread's own pixels is judged from the registers)
                const int jl = j > 0 ? j - 1 : 0, jr = j < PAN_RUN - 1 ? j + 1 : j;
                if (x > 0) {
                    unsigned k;
                    if (j > 0)
                        k = v[jl] >= 0 && !(frag >> jl & 1) ? (pan_byte(w, 3 * jl) << 8 | pan_byte(w, 3 * jl + 1)) : PC_VOID;
                    else
                        k = pa_kept_key(pan, ws, p - 1, min_area, keep_largest);
                    if (k != PC_VOID) pa_pending_add(side, t, stats, root, k);
                }
                if (x < W - 1) {
                    unsigned k;
                    if (j + 1 < n)
                        k = v[jr] >= 0 && !(frag >> jr & 1) ? (pan_byte(w, 3 * jr) << 8 | pan_byte(w, 3 * jr + 1)) : PC_VOID;
                    else
                        k = pa_kept_key(pan, ws, p + 1, min_area, keep_largest);
                    if (k != PC_VOID) pa_pending_add(side, t, stats, root, k);
                }
            }
            if (++x == W) { x = 0; ++y; }
        }
    }
    if (up.count) pa_vote(t, stats, up.root, up.key, up.count);
    if (down.count) pa_vote(t, stats, down.root, down.key, down.count);
    if (side.count) pa_vote(t, stats, side.root, side.key, side.count);
}

__global__ void __launch_bounds__(PC_T)
pa_pick_kernel(PaWs t, int *stats)
{
    // PA_PICK slots per thread, a workgroup's loads side by side
    const unsigned base = blockIdx.x * (PC_T * PA_PICK) + threadIdx.x;
    unsigned long long k[PA_PICK];
#pragma unroll
    for (int i = 0; i < PA_PICK; ++i) k[i] = base + i * PC_T < t.slots ? t.tkey[base + i * PC_T] : 0ull;
    int pairs = 0;
#pragma unroll
    for (int i = 0; i < PA_PICK; ++i) {
        if (k[i]) {
            const unsigned long long pair = k[i] - 1;
            const unsigned long long cand = (unsigned long long)t.tcount[base + i * PC_T] << 16 | (0xffffu - (unsigned)(pair & 0xffffu));
            atomicMax(&t.winner[pair >> 16], cand);       // (a count is >= 1: no candidate is 0)
            ++pairs;
        }
    }
    pairs = pc_wave_sum(pairs);
    if ((threadIdx.x & (UPS_WAVE - 1)) == 0 && pairs) atomicAdd(&stats[6], pairs);
}

// pan and out may be one buffer, as in pc_apply_kernel: the vote launch has finished with the neighbours
__global__ void __launch_bounds__(PC_T)
pa_apply_kernel(const unsigned char *pan, unsigned char *out, int *labels, const long npix, const bool vec, const int min_area,
                const int keep_largest, PcWs ws, PaWs t, int *stats)
{
    const long p0 = ((long)blockIdx.x * PC_T + threadIdx.x) * PAN_RUN;
    const bool full = stats[7] != 0;      // (written by the vote launch; this launch adds to stats[2..5] only)
    int ncomp = 0, npixels = 0, acomp = 0, apixels = 0;
    if (p0 < npix) {
        const int n = (int)min((long)PAN_RUN, npix - p0);
        unsigned w[12];
        int v[PAN_RUN];
        pan_load48(pan, p0, p0 + n, vec, w);
        pc_load_ints(ws.parent, p0, n, v);
        int prev = -1;
        bool removed = false;
        unsigned long long win = 0ull;
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j) {
            if (j < n && v[j] >= 0) {
                if (v[j] != prev) {
                    prev = v[j];
                    // (the winner cell is read beside area[], not after the verdict: a cell of a kept root holds anything, and is ignored)
                    win = t.winner[prev];
                    removed = !full && pc_removed(ws, prev, pan_byte(w, 3 * j) << 8 | pan_byte(w, 3 * j + 1), min_area, keep_largest);
                }
                if (removed) {
                    const unsigned donor = win ? 0xffffu - (unsigned)(win & 0xffffu) : 0xff00u;      // none: (255, 0)
                    const int b0 = 3 * j, b1 = 3 * j + 1;                                              // byte 2 stays
                    w[b0 >> 2] = (w[b0 >> 2] & ~(255u << (8 * (b0 & 3)))) | (donor >> 8) << (8 * (b0 & 3));
                    w[b1 >> 2] = (w[b1 >> 2] & ~(255u << (8 * (b1 & 3)))) | (donor & 255u) << (8 * (b1 & 3));
                    ++npixels;
                    ncomp += prev == (int)(p0 + j);
                    if (win) {
                        ++apixels;
                        acomp += prev == (int)(p0 + j);
                    }
                }
            }
        }
        pan_store48(out, p0, p0 + n, vec, w);
        if (labels) pc_store_ints(labels, p0, n, v);
    }
    // The four counts are reduced over the workgroup, not only over the wave: atomics on one cache line are served one after the other,
    // and four per wave of a map full of fragments took several times as long as the rest of the pass.
    __shared__ int s_count[PC_T / UPS_WAVE][4];
    ncomp = pc_wave_sum(ncomp);
    npixels = pc_wave_sum(npixels);
    acomp = pc_wave_sum(acomp);
    apixels = pc_wave_sum(apixels);
    if ((threadIdx.x & (UPS_WAVE - 1)) == 0) {
        int *c = s_count[threadIdx.x / UPS_WAVE];
        c[0] = ncomp; c[1] = npixels; c[2] = acomp; c[3] = apixels;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        int sum = 0;
#pragma unroll
        for (int i = 0; i < PC_T / UPS_WAVE; ++i) sum += s_count[i][threadIdx.x];
        if (sum) atomicAdd(&stats[2 + threadIdx.x], sum);
    }
}

// ---------------------------------------------------------------------------------------------------------------- entry points
// the argument checks of both entry points, worded with the entry point's name
static int pc_check(const char *what, const unsigned char *pan_2ch, const int height, const int width, const int connectivity,
                    const int min_area, const void *workspace, const unsigned char *out_2ch, const int *labels, const int *stats)
{
    UPS_REQUIRE(pan_2ch && workspace && out_2ch && stats, "%s: null pointer", what);
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= PC_MAX_PIXELS, "%s: image of %d x %d pixels outside 1..2^24", what,
                height, width);
    UPS_REQUIRE(connectivity == 4 || connectivity == 8, "%s: connectivity %d is neither 4 nor 8", what, connectivity);
    UPS_REQUIRE(min_area >= 0, "%s: min_area %d is negative", what, min_area);
    UPS_REQUIRE(((uintptr_t)workspace & 15) == 0 && ((uintptr_t)labels & 15) == 0 && ((uintptr_t)stats & 3) == 0,
                "%s: workspace / labels not 16-byte aligned, or stats not 4-byte aligned", what);
    return 0;
}

static int pc_label(hipStream_t st, const unsigned char *pan_2ch, const int height, const int width, const int connectivity, PcWs ws,
                    int *stats);

extern "C" size_t upsnet_pan_components_workspace_bytes(int height, int width)
{
    if (height < 1 || width < 1 || (long)height * width > PC_MAX_PIXELS) return 0;
    const long npix = (long)height * width;
    return (size_t)PC_KEYS * sizeof(unsigned long long) + (size_t)(((npix + 3) & ~3L) + npix) * sizeof(int);
}

extern "C" int upsnet_pan_components(void *stream, const unsigned char *pan_2ch, int height, int width, int connectivity, int min_area,
                                     int keep_largest, void *workspace, unsigned char *out_2ch, int *labels, int *stats)
{
    if (const int e = pc_check("pan_components", pan_2ch, height, width, connectivity, min_area, workspace, out_2ch, labels, stats)) return e;
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)height * width;
    PcWs ws = pc_ws(workspace, npix);
    if (const int e = pc_label(st, pan_2ch, height, width, connectivity, ws, stats)) return e;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const unsigned grid = (unsigned)((threads + PC_T - 1) / PC_T);
    const bool vec_in = ((uintptr_t)pan_2ch & 15) == 0;
    hipLaunchKernelGGL(pc_apply_kernel, dim3(grid), dim3(PC_T), 0, st, pan_2ch, out_2ch, labels, npix,
                       vec_in && ((uintptr_t)out_2ch & 15) == 0, min_area, keep_largest != 0, ws, stats);
    UPS_CHECK_LAUNCH("pc_apply_kernel");
    return 0;
}

extern "C" size_t upsnet_pan_absorb_workspace_bytes(int height, int width)
{
    if (height < 1 || width < 1 || (long)height * width > PC_MAX_PIXELS) return 0;
    const long npix = (long)height * width;
    return pa_winner_offset(npix) + pa_pad16(8 * (size_t)npix) + pa_table_bytes(npix);
}

extern "C" int upsnet_pan_absorb(void *stream, const unsigned char *pan_2ch, int height, int width, int connectivity, int min_area,
                                 int keep_largest, void *workspace, unsigned char *out_2ch, int *labels, int *stats)
{
    if (const int e = pc_check("pan_absorb", pan_2ch, height, width, connectivity, min_area, workspace, out_2ch, labels, stats)) return e;
    hipStream_t st = (hipStream_t)stream;
    const long npix = (long)height * width;
    PcWs ws = pc_ws(workspace, npix);
    PaWs t = pa_ws(workspace, npix);
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const unsigned grid = (unsigned)((threads + PC_T - 1) / PC_T);
    const bool vec_in = ((uintptr_t)pan_2ch & 15) == 0;
    const long nclear = (long)(pa_table_bytes(npix) / 16), clear_groups = (nclear + PC_T - 1) / PC_T;
    hipLaunchKernelGGL(pa_clear_kernel, dim3((unsigned)(clear_groups < 4096 ? clear_groups : 4096)), dim3(PC_T), 0, st, (uint4 *)t.tkey,
                       nclear, stats);
    UPS_CHECK_LAUNCH("pa_clear_kernel");
    if (const int e = pc_label(st, pan_2ch, height, width, connectivity, ws, stats)) return e;
    hipLaunchKernelGGL(pa_vote_kernel, dim3(grid), dim3(PC_T), 0, st, pan_2ch, height, width, vec_in, min_area, keep_largest != 0, ws, t,
                       stats);
    UPS_CHECK_LAUNCH("pa_vote_kernel");
    hipLaunchKernelGGL(pa_pick_kernel, dim3((t.slots + PC_T * PA_PICK - 1) / (PC_T * PA_PICK)), dim3(PC_T), 0, st, t, stats);
    UPS_CHECK_LAUNCH("pa_pick_kernel");
    hipLaunchKernelGGL(pa_apply_kernel, dim3(grid), dim3(PC_T), 0, st, pan_2ch, out_2ch, labels, npix,
                       vec_in && ((uintptr_t)out_2ch & 15) == 0, min_area, keep_largest != 0, ws, t, stats);
    UPS_CHECK_LAUNCH("pa_apply_kernel");
    return 0;
}

// The labelling launches of both entry points: tile, seam, flatten, main. Leaves parent[] flat, area[] and best[] final, stats[0..1].
static int pc_label(hipStream_t st, const unsigned char *pan_2ch, const int height, const int width, const int connectivity, PcWs ws,
                    int *stats)
{
    const long npix = (long)height * width;
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
    return 0;
}
