// pan_track.hip -- temporal association of panoptic instances across the frames of a sequence (gfx950), DESIGN.md 4.23.
//
// The reference has no tracking: the rule is this project's own and is stated in include/upsnet_hip.h and restated in plain numpy in
// tests/pan_track_ref.py. Integers throughout; the one float64 operation is the product iou_thresh * U of the candidate test.
//
// A frame is a 2-channel map (category, instance, -) as get_unified_pan_result gives it; a thing segment is (c, i), c != 255, i >= 1.
// Per pixel the tracker remembers at most one track key c << 8 | j (uint16, 0 = none). All memory pixels of one track were written by
// the same frame (a step that assigns a track rewrites its pixels under the current segment and clears every other one, and an
// unassigned track ages as a whole), so the frame index is kept once per track: stamp[key] = frame index + 1 (0 = never assigned).
//
// Three launches per frame, no host read between them:
//   pt_count_kernel    the pixel pass of pan_pixels.h with its own walk: runs of equal (current key, memory key), an LDS hash
//                      table per workgroup, one global atomic per distinct cell and workgroup (a full table falls back to the global
//                      atomic). Cells: A_cur[key], A_mem[key], I[current key][j] for equal categories. The first arrival at an A_cur
//                      cell counts the segment into nseg[c] (the row offsets of the table).
//   pt_match_kernel    one workgroup per category. Candidates (I > 0 and (double)I >= thr * (double)U) go into an LDS list: memory
//                      tracks are disjoint, so a segment has at most 1 / thr <= 16 candidates, at most 255 * 16 = 4080 per category
//                      (why thr >= 1/16 is required). The list is rank-sorted by the exact order (I1 U2 against I2 U1 in int64, ties
//                      by ascending (i, j): a strict total order, so arrival order does not matter), walked greedily by one thread,
//                      then the unmatched segments get new ids from the category's cursor, or take over the oldest unmatched track
//                      when all 255 ids are live. Writes the id map of the relabel pass, the stamps and the table rows, and
//                      zeroes every count cell of its category.
//   pt_relabel_kernel  one pass: thing pixels become (c, id, 0) and write (track, t) into the memory; any other pixel keeps its bytes,
//                      and its memory entry is cleared when its track was assigned in this step or is older than max_age.
// The head and the first host_rows rows of the table are then copied to pinned host memory on the same stream.
//
// Constant-velocity motion prediction (opt-in: upsnet_pan_track_step_motion; tests/pan_track_motion_ref.py). Every track
// also keeps the floor centroid of the pixels it was last assigned and a velocity in pixels per frame. Seven launches per frame:
//   pt_clear_kernel     zeroes the predicted memory: one 32-bit priority per pixel, 0 = none.
//   pt_predict_kernel   every real-memory pixel of track k, last assigned at frame s, votes for (x + vx (t - s), y + vy (t - s)) (the
//                       shift in int64; a vote outside the image is dropped) by atomicMax of (65535 - min(t - s, 65535)) << 16 |
//                       (65535 - k): the youngest track wins a pixel, then the smallest key, so the predicted tracks stay disjoint
//                       and the candidate bound holds. Also sets live[k]: the real memory holds k, wherever it is predicted.
//   pt_count_kernel<1>  the count pass on the predicted memory (A_mem and I are counted there).
//   pt_match_kernel<1>  "live" for id issue and the take-over pool come from live[], not from A_mem > 0: a track shifted off the image
//                       or outvoted everywhere is still remembered, and its id must not be issued twice. Leaves the old stamp of every
//                       matched track in prev[] and zeroes its category's live[].
//   pt_relabel_kernel   unchanged, on the real memory.
//   pt_moment_kernel    area, sum x and sum y (64-bit) of every track assigned in this step, from the new real memory (whose pixels
//                       of such a track are exactly the step's), pre-aggregated per workgroup in an LDS hash table.
//   pt_velocity_kernel  one thread per key: centroid = floor(sum / area); matched: v = (c_new - c_old) / (t - s) truncated toward zero,
//                       else 0. Zeroes the moment cells and prev[].
//
// pan_stable_kernel paints the frame-stable colours of a tracked map (a pure function of (category, instance)).
#include "common.h"
#include "upsnet_hip.h"
#include "pan_pixels.h"

#define PT_KEYS 65536
#define PT_HASH_BITS 11           // the count pass's LDS table: 2048 cells per workgroup
#define PT_HASH (1 << PT_HASH_BITS)
#define PT_MEM_OFF PT_KEYS        // A_mem cells
#define PT_JOINT_OFF (2 * PT_KEYS)   // I[current key][j]
#define PT_MAX_PIXELS (1L << 24)
#define PT_MAX_ROWS 65280         // 255 categories x 255 instances < 65280
#define PT_HEAD 8                 // ints before the first table row
#define PT_ROW 8                  // ints per row: c, i, id, matched, I, U, area, taken over
#define PT_MAX_CAND 4080          // 255 segments x 16 candidates
#define PTM_T 1024
#define PTM_WAVES (PTM_T / UPS_WAVE)
#define PTM_PER (4096 / PTM_T)    // candidates per thread in the rank sort (4096 >= PT_MAX_CAND)

// Workspace (ints): cnt[2 * PT_KEYS + PT_KEYS * 256] (zero between steps) | nseg[256] (zero between steps) | stamp[PT_KEYS] |
// cursor[256] | idmap[PT_KEYS] | two tables [PT_HEAD + rows * PT_ROW], rows = min(H * W, PT_MAX_ROWS): frame t fills table t & 1, so a
// table outlives the next step (the host may fetch the rows beyond those that travelled with the step's copy)
struct PtWs {
    int *cnt, *nseg, *stamp, *cursor, *idmap, *table;
};

static inline size_t pt_cnt_ints(void) { return (size_t)2 * PT_KEYS + (size_t)PT_KEYS * 256; }
static inline size_t pt_rows(long npix) { return (size_t)(npix < PT_MAX_ROWS ? npix : PT_MAX_ROWS); }
static inline size_t pt_table_ints(long npix) { return PT_HEAD + pt_rows(npix) * PT_ROW; }

static PtWs pt_ws(void *base)
{
    PtWs w;
    int *p = (int *)base;
    w.cnt = p;
    p += pt_cnt_ints();
    w.nseg = p;
    w.stamp = p + 256;
    w.cursor = w.stamp + PT_KEYS;
    w.idmap = w.cursor + 256;
    w.table = w.idmap + PT_KEYS;
    return w;
}

// Motion workspace (ints): state[PT_KEYS] as int4 (cx, cy, vx, vy) | prev[PT_KEYS] | live[PT_KEYS] | area[PT_KEYS] | sum x, sum y
// [PT_KEYS] of 64 bits each (prev .. sum y: zero between steps) | prio[H * W rounded up to 4] (the predicted memory of the last step)
#define PT_MO_COUNT_OFF (4 * PT_KEYS)
#define PT_MO_PRED_OFF (11 * PT_KEYS)
#define PT_MO_BITS 10             // the moment pass's LDS table: 1024 cells per workgroup
struct PtMo {
    int4 *state;
    int *prev, *live, *area;
    unsigned long long *sx, *sy;
    unsigned *prio;
};

static PtMo pt_mo(void *base)
{
    PtMo m;
    int *p = (int *)base;
    m.state = (int4 *)p;
    m.prev = p + PT_MO_COUNT_OFF;
    m.live = m.prev + PT_KEYS;
    m.area = m.live + PT_KEYS;
    m.sx = (unsigned long long *)(m.area + PT_KEYS);
    m.sy = m.sx + PT_KEYS;
    m.prio = (unsigned *)(p + PT_MO_PRED_OFF);
    return m;
}

static inline size_t pt_mo_ints(long npix) { return (size_t)PT_MO_PRED_OFF + (size_t)((npix + 3) & ~3L); }

__device__ static inline bool pt_is_thing(const unsigned key) { return (key >> 8) != 255 && (key & 255) != 0; }

// global count of one cell (v > 0): the first arrival at an A_cur cell counts the segment into its category
__device__ static inline void pt_global_add(const PtWs &ws, const unsigned cell, const int v)
{
    const int old = atomicAdd(&ws.cnt[cell], v);
    if (cell < PT_KEYS && old == 0) atomicAdd(&ws.nseg[cell >> 8], 1);
}

__device__ static inline void pt_add(unsigned *s_key, int *s_val, const PtWs &ws, const unsigned cell, const int v)
{
    if (!pan_lds_count<PT_HASH_BITS>(s_key, s_val, cell, v)) pt_global_add(ws, cell, v);   // LDS table full around this slot
}

// one run of `run` pixels with the same current key and memory key (0 = no entry)
__device__ static inline void pt_flush(unsigned *s_key, int *s_val, const PtWs &ws, const unsigned ck, const unsigned mk, const int run)
{
    const bool thing = pt_is_thing(ck);
    if (thing) pt_add(s_key, s_val, ws, ck, run);
    if (mk) {
        pt_add(s_key, s_val, ws, PT_MEM_OFF + mk, run);
        if (thing && (mk >> 8) == (ck >> 8)) pt_add(s_key, s_val, ws, PT_JOINT_OFF + ck * 256 + (mk & 255), run);
    }
}

// the predicted memory's keys of 16 pixels in the layout of pan_load_halves (prio is 16-byte aligned, p0 a multiple of 16)
__device__ static inline unsigned pt_pred_key(const unsigned p) { return p ? 0xffffu - (p & 0xffffu) : 0u; }

__device__ static inline void pt_load_pred(const unsigned *prio, const long p0, const long npix, unsigned w[8])
{
    if (p0 + PAN_RUN <= npix) {
        const uint4 *v = (const uint4 *)(prio + p0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 a = v[q];
            w[2 * q] = pt_pred_key(a.x) | pt_pred_key(a.y) << 16;
            w[2 * q + 1] = pt_pred_key(a.z) | pt_pred_key(a.w) << 16;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = 0;
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j)
            if (p0 + j < npix) w[j >> 1] |= pt_pred_key(prio[p0 + j]) << (16 * (j & 1));
    }
}

// MOTION: `mem` is the predicted memory (32-bit priorities), else the real one (uint16 keys)
template <bool MOTION>
__global__ void __launch_bounds__(256)
pt_count_kernel(const unsigned char *__restrict__ cur, const void *__restrict__ mem, const long npix, const bool vec, PtWs ws)
{
    __shared__ unsigned s_key[PT_HASH];
    __shared__ int s_val[PT_HASH];
    pan_lds_clear<PT_HASH_BITS>(s_key, s_val, 1);
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 < npix) {
        unsigned cw[12], mw[8];
        pan_load48(cur, p0, npix, vec, cw);
        if (MOTION) pt_load_pred((const unsigned *)mem, p0, npix, mw);
        else pan_load_halves((const unsigned short *)mem, p0, npix, vec, mw);
        unsigned pc = 0, pm = 0;
        int run = 0;
#pragma unroll
        for (int i = 0; i < PAN_RUN; ++i) {
            if (p0 + i < npix) {
                const unsigned c = pan_byte(cw, 3 * i) << 8 | pan_byte(cw, 3 * i + 1);
                const unsigned m = pan_half(mw, i);
                if (c != pc || m != pm) {
                    if (run) pt_flush(s_key, s_val, ws, pc, pm, run);
                    pc = c;
                    pm = m;
                    run = 0;
                }
                ++run;
            }
        }
        if (run) pt_flush(s_key, s_val, ws, pc, pm, run);
    }
    __syncthreads();
    pan_lds_drain<PT_HASH_BITS>(s_key, [&](const unsigned k, const int i) { pt_global_add(ws, k, s_val[i]); });
}

// a strictly precedes b: IoU descending, compared exactly (I, U <= 2^25: the products fit int64), ties by ascending (i << 8 | j)
__device__ static inline bool pt_before(const int ia, const int ua, const int ka, const int ib, const int ub, const int kb)
{
    const long long l = (long long)ia * ub, r = (long long)ib * ua;
    return l != r ? l > r : ka < kb;
}

// MOTION: A_mem and I were counted on the predicted memory; what is live comes from mo.live (set by the predict pass from the real memory)
template <bool MOTION>
__global__ void __launch_bounds__(PTM_T)
pt_match_kernel(const double thr, const int frame, PtWs ws, PtMo mo)
{
    __shared__ int s_acur[256], s_amem[256];
    __shared__ unsigned char s_live[MOTION ? 256 : 1];         // per track j: in the real memory at the start of the step
    __shared__ int s_ci[PT_MAX_CAND], s_cu[PT_MAX_CAND];      // candidates: I, U
    __shared__ unsigned short s_ck[PT_MAX_CAND];               // i << 8 | j
    __shared__ int s_id[256], s_flag[256], s_mi[256], s_mu[256], s_row[256];   // per segment i: id, matched | over << 1, I, U, row
    __shared__ unsigned char s_trk[256];                       // per track j: assigned in this step
    __shared__ int s_n, s_any;
    const int t = threadIdx.x, lane = t & (UPS_WAVE - 1), wave = t / UPS_WAVE;
    const int c = blockIdx.x;                                  // 0..254
    int *__restrict__ cnt = ws.cnt;
    if (t == 0) { s_n = 0; s_any = 0; }
    __syncthreads();
    if (t < 256) {
        const int a = t ? cnt[c << 8 | t] : 0, m = t ? cnt[PT_MEM_OFF + (c << 8 | t)] : 0;   // instance 0 is no thing; key j = 0 never stored
        s_acur[t] = a;
        s_amem[t] = m;
        s_id[t] = 0;
        s_flag[t] = 0;
        s_mi[t] = 0;
        s_mu[t] = a;
        s_trk[t] = 0;
        if (a) { cnt[c << 8 | t] = 0; s_any = 1; }
        if (m) cnt[PT_MEM_OFF + (c << 8 | t)] = 0;
        if (MOTION) {
            const int l = mo.live[c << 8 | t];
            s_live[t] = l != 0;
            if (l) mo.live[c << 8 | t] = 0;
        }
    }
    if (c == 0 && t < PT_HEAD) {                               // the table's head: number of rows, frame index
        int total = 0;
        if (t == 0) for (int k = 0; k < 255; ++k) total += ws.nseg[k];
        ws.table[t] = t == 0 ? total : (t == 1 ? frame : 0);
    }
    __syncthreads();
    if (!s_any) return;                                        // no current thing of this category: no joint cell either
    // candidates: one wave per current segment, lane l holds tracks l, l + 64, l + 128, l + 192
    for (int i = 1 + wave; i < 256; i += PTM_WAVES) {
        const int a = s_acur[i];
        if (!a) continue;
        int *__restrict__ joint = cnt + PT_JOINT_OFF + (size_t)(c << 8 | i) * 256;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = lane + UPS_WAVE * q;
            const int inter = joint[j];
            if (inter > 0) {
                joint[j] = 0;
                const int uni = a + s_amem[j] - inter;
                if ((double)inter >= thr * (double)uni) {
                    const int pos = atomicAdd(&s_n, 1);
                    if (pos < PT_MAX_CAND) { s_ci[pos] = inter; s_cu[pos] = uni; s_ck[pos] = (unsigned short)(i << 8 | j); }
                }
            }
        }
    }
    __syncthreads();
    const int n = min(s_n, PT_MAX_CAND);
    // rank sort by the exact order: every thread counts, for each of its candidates, how many precede it
    int mi[PTM_PER], mu[PTM_PER], mk[PTM_PER], rank[PTM_PER];
#pragma unroll
    for (int r = 0; r < PTM_PER; ++r) {
        const int e = t + r * PTM_T;
        mi[r] = e < n ? s_ci[e] : 0;
        mu[r] = e < n ? s_cu[e] : 1;
        mk[r] = e < n ? s_ck[e] : 0;
        rank[r] = 0;
    }
    if (n > 1) {
        for (int e = 0; e < n; ++e) {
            const int oi = s_ci[e], ou = s_cu[e], ok = s_ck[e];
#pragma unroll
            for (int r = 0; r < PTM_PER; ++r) rank[r] += pt_before(oi, ou, ok, mi[r], mu[r], mk[r]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < PTM_PER; ++r)
            if (t + r * PTM_T < n) { s_ci[rank[r]] = mi[r]; s_cu[rank[r]] = mu[r]; s_ck[rank[r]] = (unsigned short)mk[r]; }
    }
    __syncthreads();
    if (t == 0) {
        // greedy walk
        for (int e = 0; e < n; ++e) {
            const int i = s_ck[e] >> 8, j = s_ck[e] & 255;
            if (s_id[i] || s_trk[j]) continue;
            s_id[i] = j;
            s_flag[i] = 1;
            s_mi[i] = s_ci[e];
            s_mu[i] = s_cu[e];
            s_trk[j] = 1;
        }
        // new tracks in ascending i; live = in memory at the start of the step, or assigned earlier in this step
        int cursor = ws.cursor[c], row = 0;
        for (int k = 0; k < c; ++k) row += ws.nseg[k];
        for (int i = 1; i < 256; ++i) {
            if (!s_acur[i]) continue;
            s_row[i] = row++;
            if (s_id[i]) continue;
            int got = 0;
            for (int k = 0; k < 255; ++k) {
                const int id = (cursor + k) % 255 + 1;
                if (!(MOTION ? (int)s_live[id] : s_amem[id]) && !s_trk[id]) {
                    got = id;
                    cursor = (cursor + k + 1) % 255;
                    break;
                }
            }
            if (!got) {
                // all 255 ids live: take over the unassigned memory track with the oldest frame, ties to the smallest id
                int best = 0x7fffffff;
                for (int id = 1; id < 256; ++id) {
                    if (s_trk[id] || !(MOTION ? (int)s_live[id] : s_amem[id])) continue;
                    const int s = ws.stamp[c << 8 | id];
                    if (s < best) { best = s; got = id; }
                }
                s_flag[i] = 2;
            }
            s_id[i] = got;
            s_trk[got] = MOTION ? 2 : 1;                       // (2: issued or taken over, no velocity to take)
        }
        ws.cursor[c] = cursor;
    }
    __syncthreads();
    if (t >= 1 && t < 256) {
        if (s_acur[t]) {
            ws.idmap[c << 8 | t] = s_id[t];
            int *row = ws.table + PT_HEAD + (size_t)s_row[t] * PT_ROW;
            row[0] = c;
            row[1] = t;
            row[2] = s_id[t];
            row[3] = s_flag[t] & 1;
            row[4] = s_mi[t];
            row[5] = s_mu[t];
            row[6] = s_acur[t];
            row[7] = s_flag[t] >> 1;
        }
        if (MOTION && s_trk[t] == 1) mo.prev[c << 8 | t] = ws.stamp[c << 8 | t];   // matched: the frame + 1 of its last assignment
        if (s_trk[t]) ws.stamp[c << 8 | t] = frame + 1;
    }
}

__global__ void __launch_bounds__(256)
pt_relabel_kernel(const unsigned char *__restrict__ cur, unsigned char *__restrict__ out, unsigned short *__restrict__ mem, const long npix,
                  const bool vec, const int frame, const int max_age, PtWs ws)
{
    if (blockIdx.x == 0) ws.nseg[threadIdx.x] = 0;             // (256 threads; read by the match pass only, which has finished)
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    unsigned cw[12], mw[8], ow[12], kw[8];
    pan_load48(cur, p0, npix, vec, cw);
    pan_load_halves(mem, p0, npix, vec, mw);
#pragma unroll
    for (int j = 0; j < 12; ++j) ow[j] = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) kw[j] = 0;
    unsigned pc = 0xffffffffu, pm = 0xffffffffu, id = 0;
    bool thing = false, keep = false;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        const unsigned b0 = pan_byte(cw, 3 * i), b1 = pan_byte(cw, 3 * i + 1), b2 = pan_byte(cw, 3 * i + 2);
        const unsigned c = b0 << 8 | b1, m = pan_half(mw, i);   // (pixels past the end read as zeros and are not stored)
        if (c != pc) {
            pc = c;
            thing = pt_is_thing(c);
            id = thing ? (unsigned)ws.idmap[c] & 255u : 0u;
        }
        if (m != pm) {
            pm = m;
            keep = false;
            if (m) {
                const int s = ws.stamp[m];                      // frame index + 1 of the track's pixels; frame + 1: assigned in this step
                keep = s != frame + 1 && frame - (s - 1) <= max_age;
            }
        }
        const unsigned o1 = thing ? id : b1, o2 = thing ? 0u : b2;
        const unsigned k = thing ? (b0 << 8 | id) : (keep ? m : 0u);
        ow[(3 * i) >> 2] |= b0 << (8 * ((3 * i) & 3));
        ow[(3 * i + 1) >> 2] |= o1 << (8 * ((3 * i + 1) & 3));
        ow[(3 * i + 2) >> 2] |= o2 << (8 * ((3 * i + 2) & 3));
        kw[i >> 1] |= k << (16 * (i & 1));
    }
    pan_store48(out, p0, npix, vec, ow);
    pan_store_halves(mem, p0, npix, vec, kw);
}

// ------------------------------------------------------------------------------------------------- motion prediction
__global__ void __launch_bounds__(256)
pt_clear_kernel(uint4 *__restrict__ prio, const long n16)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) prio[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(256)
pt_predict_kernel(const unsigned short *__restrict__ mem, const long npix, const int width, const int height, const bool vec, const int frame,
                  const int *__restrict__ stamp, PtMo mo)
{
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    unsigned mw[8];
    pan_load_halves(mem, p0, npix, vec, mw);
    int x = (int)(p0 % width), y = (int)(p0 / width);
    unsigned pm = 0, pri = 0;
    long long dx = 0, dy = 0;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        const unsigned m = pan_half(mw, i);                    // (pixels past the end read as zeros: no vote)
        if (m != pm) {
            pm = m;
            if (m) {
                const long long age = (long long)frame - ((long long)stamp[m] - 1);
                const int4 st = mo.state[m];
                dx = (long long)st.z * age;
                dy = (long long)st.w * age;
                pri = (0xffffu - (unsigned)(age < 0 ? 0 : (age > 0xffff ? 0xffff : age))) << 16 | (0xffffu - m);
                mo.live[m] = 1;
            }
        }
        if (m) {
            const long long nx = x + dx, ny = y + dy;
            if (nx >= 0 && nx < width && ny >= 0 && ny < height) atomicMax(&mo.prio[ny * width + nx], pri);
        }
        if (++x == width) { x = 0; ++y; }
    }
}

// global moments of one key: area, sum x, sum y
__device__ static inline void pt_moment_global(const PtMo &mo, const unsigned key, const int area, const unsigned long long sx,
                                               const unsigned long long sy)
{
    atomicAdd(&mo.area[key], area);
    atomicAdd(&mo.sx[key], sx);
    atomicAdd(&mo.sy[key], sy);
}

// `mem` is the real memory after the relabel pass: the pixels of a track with stamp frame + 1 are exactly those assigned in this step
__global__ void __launch_bounds__(256)
pt_moment_kernel(const unsigned short *__restrict__ mem, const long npix, const int width, const bool vec, const int frame,
                 const int *__restrict__ stamp, PtMo mo)
{
    __shared__ unsigned s_key[1 << PT_MO_BITS];
    __shared__ int s_area[1 << PT_MO_BITS];
    __shared__ unsigned long long s_sx[1 << PT_MO_BITS], s_sy[1 << PT_MO_BITS];
    pan_lds_clear<PT_MO_BITS>(s_key, s_area, 1);
    for (int i = threadIdx.x; i < (1 << PT_MO_BITS); i += blockDim.x) { s_sx[i] = 0; s_sy[i] = 0; }
    __syncthreads();
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 < npix) {
        unsigned mw[8];
        pan_load_halves(mem, p0, npix, vec, mw);
        // one run of `run` pixels of track k on row ry from column x0: sum x = run x0 + run (run - 1) / 2, sum y = run ry
        auto flush = [&](const unsigned k, const int run, const int x0, const int ry) {
            const unsigned long long sx = (unsigned long long)run * x0 + (unsigned long long)(run * (run - 1) / 2);
            const unsigned long long sy = (unsigned long long)run * ry;
            const bool held = pan_lds_claim<PT_MO_BITS>(s_key, k, [&](const unsigned slot) {
                atomicAdd(&s_area[slot], run);
                atomicAdd(&s_sx[slot], sx);
                atomicAdd(&s_sy[slot], sy);
            });
            if (!held) pt_moment_global(mo, k, run, sx, sy);
        };
        int x = (int)(p0 % width), y = (int)(p0 / width);
        unsigned pm = 0, pk = 0;                               // pk: pm if its track was assigned in this step, else 0
        int run = 0, x0 = 0, ry = 0;
#pragma unroll
        for (int i = 0; i < PAN_RUN; ++i) {
            const unsigned m = pan_half(mw, i);                // (pixels past the end read as zeros: no run)
            if (m != pm || x == 0) {                           // a run shares its key and its row
                if (run) flush(pk, run, x0, ry);
                if (m != pm) {
                    pm = m;
                    pk = m && stamp[m] == frame + 1 ? m : 0u;
                }
                run = 0;
                x0 = x;
                ry = y;
            }
            if (pk) ++run;
            if (++x == width) { x = 0; ++y; }
        }
        if (run) flush(pk, run, x0, ry);
    }
    __syncthreads();
    pan_lds_drain<PT_MO_BITS>(s_key, [&](const unsigned k, const int i) { pt_moment_global(mo, k, s_area[i], s_sx[i], s_sy[i]); });
}

// one thread per key; a key with area > 0 was assigned in this step, prev > 0 says it was matched (frame + 1 of its last assignment)
__global__ void __launch_bounds__(256)
pt_velocity_kernel(const int frame, PtMo mo)
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;       // the grid has exactly PT_KEYS threads
    const int a = mo.area[k], prev = mo.prev[k];
    if (prev) mo.prev[k] = 0;
    if (!a) return;
    const int cx = (int)(mo.sx[k] / (unsigned long long)a), cy = (int)(mo.sy[k] / (unsigned long long)a);
    int vx = 0, vy = 0;
    if (prev) {
        const int4 old = mo.state[k];
        const int gap = max(frame - (prev - 1), 1);
        vx = (cx - old.x) / gap;                               // (C division truncates toward zero)
        vy = (cy - old.y) / gap;
    }
    mo.state[k] = make_int4(cx, cy, vx, vy);
    mo.area[k] = 0;
    mo.sx[k] = 0;
    mo.sy[k] = 0;
}

extern "C" size_t upsnet_pan_track_workspace_bytes(int height, int width)
{
    if (height < 1 || width < 1 || (long)height * width > PT_MAX_PIXELS) return 0;
    return (pt_cnt_ints() + 256 + PT_KEYS + 256 + PT_KEYS + 2 * pt_table_ints((long)height * width)) * sizeof(int);
}

extern "C" size_t upsnet_pan_track_table_offset(void) { return (pt_cnt_ints() + 256 + PT_KEYS + 256 + PT_KEYS) * sizeof(int); }

extern "C" size_t upsnet_pan_track_stamp_offset(void) { return (pt_cnt_ints() + 256) * sizeof(int); }

extern "C" size_t upsnet_pan_track_table_ints(int height, int width)
{
    if (height < 1 || width < 1 || (long)height * width > PT_MAX_PIXELS) return 0;
    return pt_table_ints((long)height * width);
}

extern "C" size_t upsnet_pan_track_motion_workspace_bytes(int height, int width)
{
    if (height < 1 || width < 1 || (long)height * width > PT_MAX_PIXELS) return 0;
    return pt_mo_ints((long)height * width) * sizeof(int);
}

extern "C" size_t upsnet_pan_track_motion_count_offset(void) { return (size_t)PT_MO_COUNT_OFF * sizeof(int); }

extern "C" size_t upsnet_pan_track_motion_pred_offset(void) { return (size_t)PT_MO_PRED_OFF * sizeof(int); }

// one step; motion_workspace = nullptr: the plain rule (three launches), else with motion prediction (seven)
static int pt_step(void *stream, const unsigned char *pan_2ch, int height, int width, double iou_thresh, int max_age, int frame,
                   void *workspace, unsigned short *memory, unsigned char *out_2ch, int *host_table, int host_rows, void *motion_workspace)
{
    UPS_REQUIRE(pan_2ch && workspace && memory && out_2ch, "pan_track_step: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width <= PT_MAX_PIXELS, "pan_track_step: image of %d x %d pixels outside 1..2^24",
                height, width);
    UPS_REQUIRE(iou_thresh >= 1.0 / 16.0 && iou_thresh <= 1.0, "pan_track_step: iou_thresh %g outside [1/16, 1]", iou_thresh);   // (NaN fails too)
    UPS_REQUIRE(max_age >= 0 && frame >= 0 && frame < 0x7ffffffe, "pan_track_step: bad max_age %d or frame index %d", max_age, frame);
    UPS_REQUIRE(host_rows >= 0, "pan_track_step: host_rows %d is negative", host_rows);
    UPS_REQUIRE(((uintptr_t)workspace & 3) == 0 && ((uintptr_t)memory & 1) == 0 && ((uintptr_t)host_table & 3) == 0,
                "pan_track_step: workspace / memory / table not aligned");
    hipStream_t st = (hipStream_t)stream;
    PtWs ws = pt_ws(workspace);
    const PtMo mo = motion_workspace ? pt_mo(motion_workspace) : PtMo{};
    const long npix = (long)height * width;
    ws.table += (size_t)(frame & 1) * pt_table_ints(npix);
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    const unsigned grid = (unsigned)((threads + 255) / 256);
    const bool vec_in = (((uintptr_t)pan_2ch | (uintptr_t)memory) & 15) == 0, vec_mem = ((uintptr_t)memory & 15) == 0;
    if (motion_workspace) {
        const long n16 = (npix + 3) / 4;
        hipLaunchKernelGGL(pt_clear_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, st, (uint4 *)mo.prio, n16);
        UPS_CHECK_LAUNCH("pt_clear_kernel");
        hipLaunchKernelGGL(pt_predict_kernel, dim3(grid), dim3(256), 0, st, memory, npix, width, height, vec_mem, frame, ws.stamp, mo);
        UPS_CHECK_LAUNCH("pt_predict_kernel");
        hipLaunchKernelGGL(pt_count_kernel<true>, dim3(grid), dim3(256), 0, st, pan_2ch, (const void *)mo.prio, npix,
                           ((uintptr_t)pan_2ch & 15) == 0, ws);
        UPS_CHECK_LAUNCH("pt_count_kernel<motion>");
        hipLaunchKernelGGL(pt_match_kernel<true>, dim3(255), dim3(PTM_T), 0, st, iou_thresh, frame, ws, mo);
        UPS_CHECK_LAUNCH("pt_match_kernel<motion>");
    } else {
        hipLaunchKernelGGL(pt_count_kernel<false>, dim3(grid), dim3(256), 0, st, pan_2ch, (const void *)memory, npix, vec_in, ws);
        UPS_CHECK_LAUNCH("pt_count_kernel");
        hipLaunchKernelGGL(pt_match_kernel<false>, dim3(255), dim3(PTM_T), 0, st, iou_thresh, frame, ws, mo);
        UPS_CHECK_LAUNCH("pt_match_kernel");
    }
    hipLaunchKernelGGL(pt_relabel_kernel, dim3(grid), dim3(256), 0, st, pan_2ch, out_2ch, memory, npix,
                       vec_in && ((uintptr_t)out_2ch & 15) == 0, frame, max_age, ws);
    UPS_CHECK_LAUNCH("pt_relabel_kernel");
    if (motion_workspace) {
        hipLaunchKernelGGL(pt_moment_kernel, dim3(grid), dim3(256), 0, st, memory, npix, width, vec_mem, frame, ws.stamp, mo);
        UPS_CHECK_LAUNCH("pt_moment_kernel");
        hipLaunchKernelGGL(pt_velocity_kernel, dim3(PT_KEYS / 256), dim3(256), 0, st, frame, mo);
        UPS_CHECK_LAUNCH("pt_velocity_kernel");
    }
    if (host_table) {
        const size_t rows = (size_t)host_rows < pt_rows(npix) ? (size_t)host_rows : pt_rows(npix);
        UPS_CHECK_HIP(hipMemcpyAsync(host_table, ws.table, (PT_HEAD + rows * PT_ROW) * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    return 0;
}

extern "C" int upsnet_pan_track_step(void *stream, const unsigned char *pan_2ch, int height, int width, double iou_thresh, int max_age,
                                     int frame, void *workspace, unsigned short *memory, unsigned char *out_2ch, int *host_table,
                                     int host_rows)
{
    return pt_step(stream, pan_2ch, height, width, iou_thresh, max_age, frame, workspace, memory, out_2ch, host_table, host_rows, nullptr);
}

extern "C" int upsnet_pan_track_step_motion(void *stream, const unsigned char *pan_2ch, int height, int width, double iou_thresh, int max_age,
                                            int frame, void *workspace, unsigned short *memory, unsigned char *out_2ch, int *host_table,
                                            int host_rows, void *motion_workspace)
{
    UPS_REQUIRE(motion_workspace && ((uintptr_t)motion_workspace & 15) == 0, "pan_track_step_motion: motion workspace null or not 16-byte aligned");
    return pt_step(stream, pan_2ch, height, width, iou_thresh, max_age, frame, workspace, memory, out_2ch, host_table, host_rows,
                   motion_workspace);
}


// ---------------------------------------------------------------------------------------------
// Frame-stable colours of a tracked map: a pure function of (category, instance), so a track keeps its colour in every frame.
//   mode 0 (PNG):     (R, G, B) = (category, instance, 1), VOID (0, 0, 0): unique within an image, id = R + 256 G + 65536 B.
//   mode 1 (picture): stuff takes the category colour; a thing takes the offset rule of pan_format.hip with ordinal := instance and
//                     the first attempt whose colour is not (0,0,0) (no taken set: colours may coincide within an image).
// cat_table as in upsnet_pan_format: -1 = unknown category (painted (0,0,0) in mode 1; the caller's table pass reports it).
#define PS_CUBE 226981u
#define PS_STEP 100003u

__device__ static inline unsigned ps_lowbias32(unsigned x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ static inline unsigned ps_clamp_add(const unsigned base, const int d)
{
    const int v = (int)base + d;
    return (unsigned)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ static inline unsigned ps_colour(const int *__restrict__ cat_table, const unsigned key, const int mode)
{
    const unsigned cat = key >> 8, inst = key & 255;
    if (cat == 255) return 0;
    if (mode == 0) return cat | inst << 8 | 1u << 16;
    const int info = cat_table[cat];
    if (info < 0) return 0;
    const unsigned base = (unsigned)info & 0xffffffu;
    if (!(info >> 24 & 1)) return base;
    const unsigned start = ps_lowbias32(cat << 16 | inst) % PS_CUBE;
    for (unsigned a = 0; a < PS_CUBE; ++a) {
        const unsigned cell = (unsigned)(((unsigned long long)start + (unsigned long long)a * PS_STEP) % PS_CUBE);
        const int dr = (int)(cell % 61) - 30, dg = (int)(cell / 61 % 61) - 30, db = (int)(cell / 3721) - 30;
        const unsigned v = ps_clamp_add(base & 255, dr) | ps_clamp_add(base >> 8 & 255, dg) << 8 | ps_clamp_add(base >> 16 & 255, db) << 16;
        if (v) return v;
    }
    return 0;
}

__global__ void __launch_bounds__(256)
pan_stable_kernel(const unsigned char *__restrict__ pred, unsigned char *__restrict__ rgb, const long npix, const bool vec,
                  const int *__restrict__ cat_table, const int mode)
{
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * PAN_RUN;
    if (p0 >= npix) return;
    unsigned w[12], o[12];
    pan_load48(pred, p0, npix, vec, w);
#pragma unroll
    for (int j = 0; j < 12; ++j) o[j] = 0;
    unsigned pk = 0xffffffffu, c = 0;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        const unsigned k = pan_byte(w, 3 * i) << 8 | pan_byte(w, 3 * i + 1);
        if (k != pk) {
            pk = k;
            c = ps_colour(cat_table, k, mode);
        }
#pragma unroll
        for (int b = 0; b < 3; ++b) o[(3 * i + b) >> 2] |= (c >> (8 * b) & 255u) << (8 * ((3 * i + b) & 3));
    }
    pan_store48(rgb, p0, npix, vec, o);
}

extern "C" int upsnet_pan_stable_colors(void *stream, const unsigned char *pred_2ch, int height, int width, const int *cat_table, int mode,
                                        unsigned char *rgb)
{
    UPS_REQUIRE(pred_2ch && rgb && (cat_table || mode == 0), "pan_stable_colors: null pointer");
    UPS_REQUIRE(height > 0 && width > 0 && (long)height * width < (1L << 31), "pan_stable_colors: bad image size %d x %d", height, width);
    UPS_REQUIRE(mode == 0 || mode == 1, "pan_stable_colors: mode %d is neither 0 (PNG) nor 1 (picture)", mode);
    const long npix = (long)height * width;
    const long threads = (npix + PAN_RUN - 1) / PAN_RUN;
    hipLaunchKernelGGL(pan_stable_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred_2ch, rgb, npix,
                       (((uintptr_t)pred_2ch | (uintptr_t)rgb) & 15) == 0, cat_table, mode);
    UPS_CHECK_LAUNCH("pan_stable_kernel");
    return 0;
}
