// pan_pixels.h -- the pixel pass every panoptic evaluator, writer and tracker begins with, stated once:
//   * a thread takes PAN_RUN = 16 pixels of a (category, instance, .) byte map into registers: three 16-byte loads when the chunk is whole
//     and the base 16-byte aligned, else byte loads; the bytes past the end of the map read as zeros and are never stored;
//   * it run-length compresses them in registers (pan_pair_walk: runs of equal (pred key, GT id[, boundary bits]); pan_row_walk: runs
//     of one key on one row) and hands every run to the caller's flush;
//   * a run's cells are counted into an LDS hash table per workgroup: 1 << BITS key words (PAN_EMPTY = free) claimed by atomicCAS,
//     linear probing over PAN_PROBES slots, the payload planes in the caller's arrays at the claimed slot;
//   * the overflow rule: when all PAN_PROBES slots around a key's home are held by other keys (noise-like maps), pan_lds_claim returns
//     false and the caller adds the run straight to its global cells; after the walk the table is drained with one global add per
//     distinct key and workgroup. Nothing is ever dropped.
// Also here: the five-plane area / bbox payload of pan_format.hip and gt_prepare.hip, and the global open-addressing cell table with
// its slot list that video_eval.hip and mots_eval.hip count a frame into.
// Everything is static inline: the library is built without relocatable device code.
#pragma once
#include "common.h"

#define PAN_KEYS 65536            // keys cat << 8 | inst of a 2-channel map (and the raw values of a 16-bit id map)
#define PAN_RUN 16                // pixels per thread
#define PAN_PROBES 16             // slots probed in an LDS table before the global fallback
#define PAN_EMPTY 0xffffffffu
#define PAN_INV 0x7fffffff        // minima are kept as the maximum of PAN_INV - value (> 0 for every coordinate)
#define PAN_TABLE_PROBES 256      // slots probed in a global cell table before it counts as full

__device__ static inline unsigned pan_hash(const unsigned key, const int bits) { return (key * 2654435761u) >> (32 - bits); }

// ------------------------------------------------------------------------------------------------------------- register chunks
__device__ static inline unsigned pan_byte(const unsigned *w, const int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255; }
__device__ static inline unsigned pan_half(const unsigned *w, const int j) { return (w[j >> 1] >> (16 * (j & 1))) & 65535; }

// 16 pixels x 3 bytes = 48 bytes per thread from src + 3 * p0. p0 == npix reads nothing. (No __restrict__ here or on pan_store48: a
// kernel that runs in place loads its chunk through one and stores it through the other.)
__device__ static inline void pan_load48(const unsigned char *src, const long p0, const long npix, const bool vec, unsigned w[12])
{
    if (vec && p0 + PAN_RUN <= npix) {
        const uint4 *v = (const uint4 *)(src + 3 * p0);
        const uint4 a = v[0], b = v[1], c = v[2];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
        w[8] = c.x; w[9] = c.y; w[10] = c.z; w[11] = c.w;
    } else {
        const long nb = 3 * (npix - p0);
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j] = 0;
#pragma unroll
        for (int j = 0; j < 3 * PAN_RUN; ++j)
            if (j < nb) w[j >> 2] |= (unsigned)src[3 * p0 + j] << (8 * (j & 3));
    }
}

__device__ static inline void pan_store48(unsigned char *dst, const long p0, const long npix, const bool vec, const unsigned w[12])
{
    if (vec && p0 + PAN_RUN <= npix) {
        uint4 *v = (uint4 *)(dst + 3 * p0);
        v[0] = make_uint4(w[0], w[1], w[2], w[3]);
        v[1] = make_uint4(w[4], w[5], w[6], w[7]);
        v[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
        const long nb = 3 * (npix - p0);
#pragma unroll
        for (int j = 0; j < 3 * PAN_RUN; ++j)
            if (j < nb) dst[3 * p0 + j] = (unsigned char)pan_byte(w, j);
    }
}

// 16 uint16 per thread: two 16-byte accesses or element accesses
__device__ static inline void pan_load_halves(const unsigned short *src, const long p0, const long npix, const bool vec, unsigned w[8])
{
    if (vec && p0 + PAN_RUN <= npix) {
        const uint4 *v = (const uint4 *)(src + p0);
        const uint4 a = v[0], b = v[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
        w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) w[j] = 0;
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j)
            if (p0 + j < npix) w[j >> 1] |= (unsigned)src[p0 + j] << (16 * (j & 1));
    }
}

__device__ static inline void pan_store_halves(unsigned short *dst, const long p0, const long npix, const bool vec, const unsigned w[8])
{
    if (vec && p0 + PAN_RUN <= npix) {
        uint4 *v = (uint4 *)(dst + p0);
        v[0] = make_uint4(w[0], w[1], w[2], w[3]);
        v[1] = make_uint4(w[4], w[5], w[6], w[7]);
    } else {
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j)
            if (p0 + j < npix) dst[p0 + j] = (unsigned short)pan_half(w, j);
    }
}

// 16 bytes per thread: one 16-byte load or byte loads
__device__ static inline void pan_load16(const unsigned char *src, const long p0, const long npix, const bool vec, unsigned w[4])
{
    if (vec && p0 + PAN_RUN <= npix) {
        const uint4 v = *(const uint4 *)(src + p0);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = 0;
#pragma unroll
        for (int j = 0; j < PAN_RUN; ++j)
            if (p0 + j < npix) w[j >> 2] |= (unsigned)src[p0 + j] << (8 * (j & 3));
    }
}

// ------------------------------------------------------------------------------------------------------------- LDS hash table
// every thread of the workgroup: all keys free, `planes` payload planes of 1 << BITS words zero (the caller synchronises)
template <int BITS, class T>
__device__ static inline void pan_lds_clear(unsigned *s_key, T *s_val, const int planes)
{
    for (int i = threadIdx.x; i < (1 << BITS); i += blockDim.x) s_key[i] = PAN_EMPTY;
    for (int i = threadIdx.x; i < planes << BITS; i += blockDim.x) s_val[i] = 0;
}

// Finds or claims the slot of `key` in the workgroup's table and calls add(slot) there; false: full around the key's home, nothing
// was added and the caller adds globally. (The add sits inside the probe loop, not behind a returned slot: the compiler then keeps the
// hit path free of the fallback's test, which measured 2-4 % of these kernels.)
template <int BITS, class F>
__device__ static inline bool pan_lds_claim(unsigned *s_key, const unsigned key, F add)
{
    const unsigned h = pan_hash(key, BITS);
    for (int p = 0; p < PAN_PROBES; ++p) {
        const unsigned slot = (h + p) & ((1u << BITS) - 1);
        unsigned k = __hip_atomic_load(&s_key[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == PAN_EMPTY) k = atomicCAS(&s_key[slot], PAN_EMPTY, key);
        if (k == PAN_EMPTY || k == key) {
            add(slot);
            return true;
        }
    }
    return false;
}

// one count plane
template <int BITS>
__device__ static inline bool pan_lds_count(unsigned *s_key, int *s_val, const unsigned key, const int v)
{
    return pan_lds_claim<BITS>(s_key, key, [&](const unsigned slot) { atomicAdd(&s_val[slot], v); });
}

// every thread of the workgroup, after the walk and a __syncthreads(): add(key, slot) once per key the table holds
template <int BITS, class F>
__device__ static inline void pan_lds_drain(const unsigned *s_key, F add)
{
    for (int i = threadIdx.x; i < (1 << BITS); i += blockDim.x) {
        const unsigned k = s_key[i];
        if (k != PAN_EMPTY) add(k, i);
    }
}

// ------------------------------------------------------------------------------------------------------------- the walks
// Runs of equal (pred key cat << 8 | inst, 24-bit GT id[, low two bits of `bits`]) among the thread's pixels p0 .. p0 + 15 (p0 < npix):
// flush(pred key, GT id, bits, run length), bits = 0 without BITS. `bits` is one byte per pixel and 16-byte aligned.
template <bool BITS, class F>
__device__ static inline void pan_pair_walk(const unsigned char *pred, const unsigned char *gt, const unsigned char *bits, const long p0,
                                            const long npix, const bool vec, F flush)
{
    unsigned pw[12], gw[12], bw[4];
    pan_load48(pred, p0, npix, vec, pw);
    pan_load48(gt, p0, npix, vec, gw);
    if (BITS) pan_load16(bits, p0, npix, true, bw);
    unsigned pk = 0, bb = 0;
    int gid = -1, run = 0;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        if (p0 + i < npix) {
            const unsigned k = pan_byte(pw, 3 * i) << 8 | pan_byte(pw, 3 * i + 1);
            const int g = (int)(pan_byte(gw, 3 * i) | pan_byte(gw, 3 * i + 1) << 8 | pan_byte(gw, 3 * i + 2) << 16);
            const unsigned b = BITS ? pan_byte(bw, i) & 3 : 0u;
            if (k != pk || g != gid || b != bb) {
                if (run) flush(pk, gid, bb, run);
                pk = k;
                gid = g;
                bb = b;
                run = 0;
            }
            ++run;
        }
    }
    if (run) flush(pk, gid, bb, run);
}

// Runs of one key on one row: flush(key, run length, first column, row)
template <class F>
__device__ static inline void pan_row_walk(const unsigned char *pred, const long p0, const long npix, const int width, const bool vec, F flush)
{
    unsigned w[12];
    pan_load48(pred, p0, npix, vec, w);
    int x = (int)(p0 % width), y = (int)(p0 / width);
    unsigned pk = 0;
    int run = 0, x0 = 0, ry = 0;
#pragma unroll
    for (int i = 0; i < PAN_RUN; ++i) {
        if (p0 + i < npix) {
            const unsigned k = pan_byte(w, 3 * i) << 8 | pan_byte(w, 3 * i + 1);
            if (run == 0 || k != pk || x == 0) {   // a run shares its key and its row
                if (run) flush(pk, run, x0, ry);
                pk = k;
                run = 0;
                x0 = x;
                ry = y;
            }
            ++run;
            if (++x == width) { x = 0; ++y; }
        }
    }
    if (run) flush(pk, run, x0, ry);
}

// ------------------------------------------------------------------------------------------------------------- area / bbox payload
// Five planes of PAN_KEYS ints from `cells`: area | PAN_INV - x_min | PAN_INV - y_min | x_max | y_max; a zeroed cell is "nothing yet"
// for all five. The LDS table carries the same five planes, 1 << BITS ints each.
__device__ static inline void pan_box_global_add(int *cells, const unsigned key, const int area, const int nx, const int ny, const int xm,
                                                 const int ym)
{
    atomicAdd(&cells[key], area);
    atomicMax(&cells[PAN_KEYS + key], nx);
    atomicMax(&cells[2 * PAN_KEYS + key], ny);
    atomicMax(&cells[3 * PAN_KEYS + key], xm);
    atomicMax(&cells[4 * PAN_KEYS + key], ym);
}

// one run of `run` pixels of one key on row y, columns x0 .. x0 + run - 1: its bbox share is its two end columns and its row
template <int BITS>
__device__ static inline void pan_box_add(unsigned *s_key, int *s_val, int *cells, const unsigned key, const int run, const int x0, const int y)
{
    const int x1 = x0 + run - 1;
    const bool held = pan_lds_claim<BITS>(s_key, key, [&](const unsigned slot) {
        atomicAdd(&s_val[slot], run);
        atomicMax(&s_val[(1 << BITS) + slot], PAN_INV - x0);
        atomicMax(&s_val[(2 << BITS) + slot], PAN_INV - y);
        atomicMax(&s_val[(3 << BITS) + slot], x1);
        atomicMax(&s_val[(4 << BITS) + slot], y);
    });
    if (!held) pan_box_global_add(cells, key, run, PAN_INV - x0, PAN_INV - y, x1, y);
}

template <int BITS>
__device__ static inline void pan_box_drain(const unsigned *s_key, const int *s_val, int *cells)
{
    pan_lds_drain<BITS>(s_key, [&](const unsigned k, const int i) {
        pan_box_global_add(cells, k, s_val[i], s_val[(1 << BITS) + i], s_val[(2 << BITS) + i], s_val[(3 << BITS) + i], s_val[(4 << BITS) + i]);
    });
}

// ------------------------------------------------------------------------------------------------------------- global cell table
// Open addressing in global memory: uint[2 << bits], slot = (cell + 1, count), 0 = empty, claimed by atomicCAS; the claimer appends its
// slot to `slots` at *counter, so nothing ever scans a table. Sized per frame: 2^12 .. 2^20 slots, about one per 16 pixels.
static inline int pan_frame_bits(long npix)
{
    int b = 12;
    while (b < 20 && (1L << b) < npix / 16) ++b;
    return b;
}

// count v > 0 of one cell; PAN_TABLE_PROBES slots in a row taken: full_bit of *status is set, never silently
__device__ static inline void pan_table_add(unsigned *tab, const int bits, int *slots, int *counter, unsigned long long *status,
                                            const unsigned long long full_bit, const unsigned cell, const unsigned v)
{
    const unsigned mask = (1u << bits) - 1, want = cell + 1;
    unsigned slot = pan_hash(cell, bits);
    for (int p = 0; p < PAN_TABLE_PROBES; ++p, slot = (slot + 1) & mask) {
        unsigned k = __hip_atomic_load(&tab[2 * slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            k = atomicCAS(&tab[2 * slot], 0u, want);
            if (k == 0) {
                const int pos = atomicAdd(counter, 1);
                if (pos >= 0 && pos <= (int)mask) slots[pos] = (int)slot;   // one append per slot: always true for a zeroed workspace
                k = want;
            }
        }
        if (k == want) {
            atomicAdd(&tab[2 * slot + 1], v);
            return;
        }
    }
    atomicOr(status, full_bit);   // the host raises at its next synchronisation
}

// the count of a cell of a finished table (0 if it has none)
__device__ static inline unsigned pan_table_lookup(const unsigned *tab, const int bits, const unsigned cell)
{
    const unsigned mask = (1u << bits) - 1, want = cell + 1;
    unsigned slot = pan_hash(cell, bits);
    for (int p = 0; p < PAN_TABLE_PROBES; ++p, slot = (slot + 1) & mask) {
        const unsigned k = tab[2 * slot];
        if (k == want) return tab[2 * slot + 1];
        if (k == 0) return 0u;
    }
    return 0u;
}
