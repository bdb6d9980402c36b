// residency.h -- cap on the workgroups of one kernel that live on a CU at a time, enforced by the LAUNCH alone.
//
// Why: with two images in flight (one HIP graph instance per stream, models/resnet_upsnet.py) the kernels of one image are meant to run
// under the lock-step phases of the other's (prologue, first-operand wait, epilogue: DESIGN.md 4.1 (ii)). Every hot launch fills a CU
// by itself -- registers or LDS -- so a workgroup of the other image's kernel enters a CU only when a whole workgroup retires. A cap
// below a kernel's own residency leaves registers, wave slots and LDS of every CU to whatever else is runnable.
//
// How: the hardware admits floor(LDS per CU / LDS per workgroup) workgroups, so the launcher asks for more dynamic LDS than the kernel
// uses. The kernel never touches the padding: code, arithmetic and results are those of the uncapped launch, bit for bit. The request
// is the SMALLEST that admits `cap` and not `cap + 1` workgroups, so that the rest of the CU's LDS stays free for the partner kernel.
// Two kernels that are both capped this way cannot share a CU at their caps (a / (a + 1) + b / (b + 1) >= 1 for a, b >= 1): a capped
// kernel pairs with an uncapped one, which takes what registers and LDS are left.
#pragma once
#include <cstddef>

enum ResKernel {
    RES_CONV1X1_FRAG = 0,   // conv1x1_frag_f32_kernel, every mode          4 workgroups x 4 waves x 128 registers, 16 KiB
    RES_CONV1X1_PAIR,       // conv1x1_pair_f32_kernel (res2 / res3 forms)  3 x 4 x 142, 50 / 65 KiB
    RES_CONV1X1_PAIR32,     // conv1x1_pair32_f32_kernel (res4 form)        66 / 50 KiB
    RES_CONV1X1_KSW,        // conv1x1_ksw_f32_kernel, every tile           2 .. 6 workgroups by registers, static LDS only
    RES_WINO16_32X64,       // conv_wino16_f32_kernel<., 32, 64>            2 x 4 x 219, 64 KiB
    RES_WINO16_32X32,       // conv_wino16_f32_kernel<., 32, 32>            2, 64 KiB
    RES_DCN_FUSED,          // dcn_fused_f32_kernel                         3 x 4 x 122-138, ~50 KiB
    RES_NKERNELS
};

#define RES_LDS_PER_CU 163840    // gfx950: 160 KiB per CU, also the most one workgroup may ask for
#define RES_LDS_GRANULE 1280     // allocation granule (320 dwords): a request is rounded up to it
#define RES_MAX_CAP 8            // (the padding below is exact while cap (cap + 1) granules <= LDS per CU: cap <= 10)

// Dynamic LDS to ADD to a launch whose workgroup uses static_lds + dynamic_lds bytes so that exactly `cap` workgroups fit a CU
// (fewer if the kernel's own footprint -- LDS here, registers in general -- already admits fewer: then nothing is added). 0 for cap 0.
static inline size_t res_pad_bytes(int cap, size_t static_lds, size_t dynamic_lds)
{
    if (cap <= 0) return 0;
    if (cap > RES_MAX_CAP) cap = RES_MAX_CAP;
    const size_t own = (static_lds + dynamic_lds + RES_LDS_GRANULE - 1) / RES_LDS_GRANULE * RES_LDS_GRANULE;
    // smallest granule multiple above LDS / (cap + 1): cap + 1 workgroups of it no longer fit
    const size_t want = ((size_t)RES_LDS_PER_CU / (cap + 1) / RES_LDS_GRANULE + 1) * RES_LDS_GRANULE;
    if (own >= want) return 0;                       // the kernel's own LDS already holds it to cap or fewer
    return want - static_lds - dynamic_lds;          // static + dynamic + pad == want <= LDS / cap
}

// the table (conv.hip): g_res_cap[k] = 0 today's launch, n >= 1 at most n workgroups per CU
extern int g_res_cap[RES_NKERNELS];
extern int g_res_last_dynamic;   // dynamic LDS of the most recent covered launch (tests: the cap did reach the launch)

// dynamic LDS a covered launcher passes to the launch: its own plus the padding of the kernel's cap
static inline size_t res_dynamic_lds(int kernel, size_t static_lds, size_t dynamic_lds)
{
    const size_t d = dynamic_lds + res_pad_bytes(g_res_cap[kernel], static_lds, dynamic_lds);
    g_res_last_dynamic = (int)d;
    return d;
}

// the most dynamic LDS a capped launch of a kernel with `static_lds` bytes of static LDS can ask for (hipFuncAttributeMaxDynamicSharedMemorySize:
// set once per device in the eager forwards, so that a launch under stream capture never has to change a function attribute)
static inline int res_max_dynamic(size_t static_lds) { return (int)(RES_LDS_PER_CU - static_lds); }
