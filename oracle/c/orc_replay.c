/*
 * orc_replay.c -- TEST INFRASTRUCTURE ONLY: replays one recorded call of an orc_* function of upsnet_oracle.c in a process of
 * its own, so that the restatement can be run under AddressSanitizer / UndefinedBehaviorSanitizer (oracle.build_replay,
 * tests/test_oracle_sanitized_cpu.py) and compared bit for bit across builds, fill patterns and thread counts.
 *
 *     orc_replay CASE RESULT
 *
 * Case file, little-endian (written by oracle/replay.py with numpy only):
 *     u32 magic 'ORCR' (0x5243524f), u32 function id (the table below), u32 fill byte, u32 threads, u32 record count,
 *     then one record per C argument, in argument order:
 *         u32 role  0 = input, 1 = output, 2 = in/out, 3 = NULL pointer
 *         u32 dtype 0 = f32, 1 = i32, 2 = i64, 3 = u8, 4 = f64, 5 = u32
 *         u32 ndim, i64 dims[ndim]            (ndim 0: a scalar argument, passed by value)
 *         raw bytes of the array              (roles 0 and 2 only)
 * Every array, input or output, is malloc'ed at exactly its stated size, so that a read or write one element past it lands in
 * a redzone; an output is filled with the case's fill byte before the call, so that an element the function never writes shows.
 * Result file: i32 integer return value (0 for void), f32 float return value (0 otherwise), then the raw bytes of every role 1
 * and role 2 record in argument order.
 */
#include <stdio.h>

#include "upsnet_oracle.c"

#define ORC_MAXREC 32

typedef struct {
    uint32_t role, dtype, ndim;
    size_t bytes;
    void *ptr;
} orc_rec;

static const size_t orc_dtype_size[6] = {4, 4, 8, 1, 8, 4};
static orc_rec rec[ORC_MAXREC];
static uint32_t nrec;

static void die(const char *what)
{
    fprintf(stderr, "orc_replay: %s\n", what);
    exit(2);
}

static void need(FILE *f, void *dst, size_t n)
{
    if (n && fread(dst, 1, n, f) != n) die("case file is truncated");
}

static void *arg(uint32_t i, uint32_t dtype, int scalar)
{
    if (i >= nrec) die("too few records for this function");
    if (rec[i].role == 3) {
        if (scalar) die("NULL given for a scalar argument");
        return NULL;
    }
    if (rec[i].dtype != dtype) die("record has the wrong dtype for its argument");
    if (scalar && (rec[i].ndim != 0 || rec[i].role != 0)) die("scalar argument expected");
    if (!scalar && rec[i].ndim == 0) die("array argument expected");
    return rec[i].ptr;
}

#define PF(i) ((float *)arg(i, 0, 0))
#define PI(i) ((int *)arg(i, 1, 0))
#define PL(i) ((int64_t *)arg(i, 2, 0))
#define PB(i) ((uint8_t *)arg(i, 3, 0))
#define PD(i) ((double *)arg(i, 4, 0))
#define I(i) (*(int *)arg(i, 1, 1))
#define F(i) (*(float *)arg(i, 0, 1))
#define D(i) (*(double *)arg(i, 4, 1))
#define U(i) (*(unsigned *)arg(i, 5, 1))

int main(int argc, char **argv)
{
    if (argc != 3) die("usage: orc_replay CASE RESULT");
    FILE *f = fopen(argv[1], "rb");
    if (!f) die("cannot open the case file");
    uint32_t head[5];
    need(f, head, sizeof head);
    if (head[0] != 0x5243524fu) die("bad magic");
    const uint32_t func = head[1], fill = head[2], threads = head[3];
    nrec = head[4];
    if (nrec > ORC_MAXREC) die("too many records");
    for (uint32_t i = 0; i < nrec; ++i) {
        uint32_t h[3];
        need(f, h, sizeof h);
        rec[i].role = h[0]; rec[i].dtype = h[1]; rec[i].ndim = h[2];
        if (h[0] > 3 || h[1] > 5 || h[2] > 8) die("bad record header");
        size_t count = 1;
        for (uint32_t d = 0; d < h[2]; ++d) {
            int64_t dim;
            need(f, &dim, sizeof dim);
            if (dim < 0 || dim > (1 << 28)) die("bad dimension");
            count *= (size_t)dim;
        }
        rec[i].bytes = count * orc_dtype_size[h[1]];
        rec[i].ptr = NULL;
        if (h[0] == 3) continue;
        rec[i].ptr = malloc(rec[i].bytes);
        if (!rec[i].ptr) die("out of memory");
        if (h[0] == 1) memset(rec[i].ptr, (int)fill, rec[i].bytes);
        else need(f, rec[i].ptr, rec[i].bytes);
    }
    fclose(f);

    orc_set_threads((int)threads);
    int32_t iret = 0;
    float fret = 0.f;
    switch (func) {
    case 1: orc_roi_align_forward(PF(0), I(1), I(2), I(3), PF(4), I(5), I(6), I(7), I(8), F(9), PF(10)); break;
    case 2: orc_deform_im2col(PF(0), PF(1), PF(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), I(10), I(11), I(12), I(13), I(14), PF(15)); break;
    case 3: orc_roi_align_backward(PF(0), PF(1), I(2), I(3), I(4), I(5), I(6), I(7), I(8), F(9), PF(10)); break;
    case 4: orc_deform_col2im(PF(0), PF(1), PF(2), I(3), I(4), I(5), I(6), I(7), I(8), I(9), I(10), I(11), I(12), I(13), I(14), I(15), I(16), I(17), PF(18)); break;
    case 5: orc_deform_col2im_coord(PF(0), PF(1), PF(2), PF(3), I(4), I(5), I(6), I(7), I(8), I(9), I(10), I(11), I(12), I(13), I(14), I(15), I(16), I(17), I(18), PF(19), PF(20)); break;
    case 6: iret = orc_nms_sorted(PF(0), I(1), I(2), F(3), PI(4)); break;
    case 7: iret = orc_cpu_nms_sorted(PF(0), I(1), I(2), D(3), PI(4)); break;
    case 8: iret = orc_soft_nms(PF(0), PL(1), I(2), F(3), F(4), F(5), U(6)); break;
    case 9: fret = orc_resize_at(PF(0), I(1), I(2), I(3), I(4), I(5)); break;
    case 10: orc_resize_bilinear(PF(0), I(1), I(2), I(3), PF(4)); break;
    case 11: iret = orc_mask_removal(PF(0), PF(1), PL(2), PL(3), I(4), I(5), I(6), I(7), I(8), D(9), PB(10), PL(11), PF(12)); break;
    case 12: orc_seg_term(PF(0), I(1), I(2), I(3), PF(4), PL(5), PL(6), I(7), PF(8)); break;
    case 13: orc_panoptic_fuse(PF(0), I(1), I(2), I(3), I(4), PF(5), PF(6), I(7), I(8), PL(9), PL(10)); break;
    case 14: orc_upsample_bilinear(PF(0), I(1), I(2), I(3), I(4), PF(5)); break;
    case 15: {
        /* argument 0 of orc_fcn_score_combine is an array of nlev pointers: the case carries (nlev, S, H, W, bias, out) and then the nlev maps */
        const int nlev = I(0);
        const float *part[ORC_MAXREC];
        if (nlev < 1 || 6 + (uint32_t)nlev != nrec) die("fcn_score_combine: record count does not match nlev");
        for (int l = 0; l < nlev; ++l) part[l] = PF(6 + (uint32_t)l);
        orc_fcn_score_combine(part, nlev, I(1), I(2), I(3), PF(4), PF(5));
        break;
    }
    case 16: orc_prep_image(PB(0), I(1), I(2), PD(3), D(4), I(5), I(6), I(7), I(8), PF(9)); break;
    case 17: orc_set_threads(I(0)); break;
    default: die("unknown function id");
    }

    f = fopen(argv[2], "wb");
    if (!f) die("cannot open the result file");
    fwrite(&iret, sizeof iret, 1, f);
    fwrite(&fret, sizeof fret, 1, f);
    for (uint32_t i = 0; i < nrec; ++i)
        if ((rec[i].role == 1 || rec[i].role == 2) && rec[i].bytes) fwrite(rec[i].ptr, 1, rec[i].bytes, f);
    if (fclose(f) != 0) die("cannot write the result file");
    for (uint32_t i = 0; i < nrec; ++i) free(rec[i].ptr);
    return 0;
}
