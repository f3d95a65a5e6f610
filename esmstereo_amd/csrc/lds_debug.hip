// Diagnostics for the one memory no test can reach from the host: LDS.  The hardware does not clear it between
// workgroups or launches, so a kernel that reads a cell it never wrote reads what the previous kernel on that CU left
// there.  These two launches let a test choose what that is (tests/lds_poison.py):
//
//  esm_lds_fill_u32   writes one 32-bit pattern into all 163,840 B of every CU's LDS.  A workgroup declares the whole
//    160 KiB, so at most one is resident per CU, and the grid is kLdsWgPerCu workgroups per CU, so the dispatcher has
//    to use every CU.  No grid-wide barrier and no counter to spin on: workgroups that are not resident yet would hang
//    either.  Each thread reads one word back (a word another thread stored) and reports a mismatch through an ordinary
//    global store, which keeps the LDS stores observable.
//  esm_lds_probe_u32  the same geometry, and no LDS store at all: each workgroup counts the words of its 160 KiB that
//    differ from the pattern and writes (count, CU identity) to out[2 wg], out[2 wg + 1].  It is a kernel whose
//    output depends on leftovers only, the positive control of the harness.  The LDS is dynamic (extern __shared__):
//    loads from a static __shared__ array that nothing stores to are folded away at compile time.  One wave does
//    the counting with wave-wide ballots, whose sums are uniform and need no LDS to combine.
//  CU identity: XCC_ID's id field above HW_ID's CU / SH / SE fields (read-only s_getreg).
#include "common.h"

namespace esm {
namespace {

constexpr int kLdsBytes = 163840;
constexpr int kLdsWords = kLdsBytes / 4;
constexpr int kLdsThreads = 256;
constexpr int kLdsWgPerCu = 8;

__device__ uint32_t g_lds_sink;  // receives a word the fill read back wrong (never, on working hardware)

__global__ __launch_bounds__(kLdsThreads) void lds_fill_kernel(uint32_t pattern) {
    __shared__ uint32_t lds[kLdsWords];
    volatile uint32_t* p = lds;
    const int tid = static_cast<int>(threadIdx.x);
    for (int i = tid; i < kLdsWords; i += kLdsThreads) p[i] = pattern;
    __syncthreads();
    const uint32_t v = p[(tid * (kLdsWords / kLdsThreads) + 64 + 1) % kLdsWords];  // stored by another thread
    if (v != pattern) g_lds_sink = v;
}

__global__ __launch_bounds__(kLdsThreads) void lds_probe_kernel(uint32_t pattern, uint32_t* __restrict__ out) {
    extern __shared__ uint32_t dyn_lds[];
    const int tid = static_cast<int>(threadIdx.x);
    if (tid >= 64) return;
    uint32_t bad = 0;
    for (int i = tid; i < kLdsWords; i += 64)
        bad += static_cast<uint32_t>(__popcll(__ballot(dyn_lds[i] != pattern)));
    if (tid == 0) {
        const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_ID: CU [11:8], SH [12], SE [15:13]
        const uint32_t xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20);   // XCC_ID: id [3:0]
        out[2 * blockIdx.x] = bad;
        out[2 * blockIdx.x + 1] = (xcc << 16) | (hw & 0xff00u);
    }
}

// kLdsWgPerCu workgroups per CU of the current device, or a negative status
int lds_grid() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        set_error("lds diagnostics: no device to read the CU count of");
        return ESM_ERR_RUNTIME;
    }
    return kLdsWgPerCu * cus;
}

}  // namespace
}  // namespace esm

extern "C" {

int esm_lds_probe_workgroups(void) { return esm::lds_grid(); }

int esm_lds_fill_u32(uint32_t pattern, void* stream) {
    const int grid = esm::lds_grid();
    if (grid < 0) return grid;
    hipLaunchKernelGGL(esm::lds_fill_kernel, dim3(grid), dim3(esm::kLdsThreads), 0, esm::as_stream(stream), pattern);
    return esm::check_launch("lds_fill");
}

int esm_lds_probe_u32(uint32_t pattern, uint32_t* out, int n_workgroups, void* stream) {
    if (!out) return esm::arg_error("lds_probe: null out");
    // (the grid is at least kLdsWgPerCu workgroups on any device: refused before the device is asked)
    if (n_workgroups < esm::kLdsWgPerCu) return esm::arg_error("lds_probe: n_workgroups below esm_lds_probe_workgroups()");
    const int grid = esm::lds_grid();
    if (grid < 0) return grid;
    if (n_workgroups < grid) return esm::arg_error("lds_probe: n_workgroups below esm_lds_probe_workgroups()");
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(esm::lds_probe_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, esm::kLdsBytes) != hipSuccess) {
        (void)hipGetLastError();
        esm::set_error("lds_probe: the device refuses 160 KiB of dynamic LDS");
        return ESM_ERR_RUNTIME;
    }
    hipLaunchKernelGGL(esm::lds_probe_kernel, dim3(grid), dim3(esm::kLdsThreads), esm::kLdsBytes, esm::as_stream(stream),
                       pattern, out);
    return esm::check_launch("lds_probe");
}

}  // extern "C"
