// What the first-load records share (conv_lean_rec.h, conv_pair2_rec.h, conv_c1_rec.h).  A record is N
// leading `unsigned` kernel arguments, so that one scalar load brings all that a workgroup's first loads need; its
// layout, field limits and refusal rules are its own header's.
#pragma once

#include <initializer_list>

#include "common.h"

namespace esm {
namespace conv {

// floor(n / d) as the high word of n * m, m = magic_u32(d) = ceil(2^32 / d) from the host.  Exact while
// n * (d - 1) < 2^32: m * d = 2^32 + e with 0 <= e <= d - 1, so n * m / 2^32 = n / d + n * e / (d * 2^32); with
// n = q * d + r the floor stays q while r + n * e / 2^32 < d, and the worst case r = e = d - 1 asks for
// n * (d - 1) < 2^32 (n * d <= 2^32 is enough).  m = 0 stands for d = 1, whose 2^32 does not fit.
inline unsigned magic_u32(long long d) {
    return d <= 1 ? 0u : static_cast<unsigned>(((1ull << 32) + static_cast<unsigned long long>(d) - 1) / d);
}
__host__ __device__ __forceinline__ unsigned magic_div(unsigned n, unsigned m) {
#ifdef __HIP_DEVICE_COMPILE__
    return m ? __umulhi(n, m) : n;
#else
    return m ? static_cast<unsigned>(static_cast<unsigned long long>(n) * m >> 32) : n;
#endif
}
__host__ __device__ __forceinline__ int magic_div(int n, unsigned m) {
    return static_cast<int>(magic_div(static_cast<unsigned>(n), m));
}

// a pointer as two record dwords, and back; as a hook's int64 field
inline int64_t ptr_field(const void* p) { return static_cast<int64_t>(reinterpret_cast<uintptr_t>(p)); }
inline unsigned ptr_lo(const void* p) { return static_cast<unsigned>(reinterpret_cast<unsigned long long>(p)); }
inline unsigned ptr_hi(const void* p) { return static_cast<unsigned>(reinterpret_cast<unsigned long long>(p) >> 32); }
__host__ __device__ inline const float* ptr_join(unsigned lo, unsigned hi) {
    return reinterpret_cast<const float*>(static_cast<unsigned long long>(hi) << 32 | lo);
}

// every stride (elements) fits a record dword as a non-negative int
inline bool strides_fit(std::initializer_list<int64_t> strides) {
    for (const int64_t st : strides)
        if (st < 0 || st >= (1ll << 31)) return false;
    return true;
}

// The BN constants sit behind c's nw packed weights as engine.pack_conv lays them, [taps][cin_pad][cout_pad] | scale |
// shift, so that a kernel reads them through the weight pointer; scale_optional: a descriptor without a scale passes
inline bool bn_behind_weights(const esm_conv_desc& c, long long nw, bool scale_optional) {
    if (!c.w || !c.shift || c.shift != c.w + nw + c.cout_pad) return false;
    return c.scale ? c.scale == c.w + nw : scale_optional;
}

// The test hooks' way out (esm_*_record_pack): the record's dwords and its unpacked fields, copied to the caller
template <int ND, int NF>
inline int record_export(const unsigned (&d)[ND], const int64_t (&f)[NF], uint32_t* rec, int64_t* fields) {
    for (int i = 0; i < ND; ++i) rec[i] = d[i];
    for (int i = 0; i < NF; ++i) fields[i] = f[i];
    return 1;
}

// The N dwords (N = 14, 16, 20) as a kernel's leading parameters r0 .. rN-1, as the brace list a *_record_unpack
// takes, and as launch arguments from an array: separate `unsigned` parameters, in order, at byte offsets 4 i.
#define ESM_REC_PARAMS_14                                                                                       \
    unsigned r0, unsigned r1, unsigned r2, unsigned r3, unsigned r4, unsigned r5, unsigned r6, unsigned r7,     \
        unsigned r8, unsigned r9, unsigned r10, unsigned r11, unsigned r12, unsigned r13
#define ESM_REC_PARAMS_16 ESM_REC_PARAMS_14, unsigned r14, unsigned r15
#define ESM_REC_PARAMS_20 ESM_REC_PARAMS_16, unsigned r16, unsigned r17, unsigned r18, unsigned r19
#define ESM_REC_DWORDS_14 r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13
#define ESM_REC_DWORDS_16 ESM_REC_DWORDS_14, r14, r15
#define ESM_REC_DWORDS_20 ESM_REC_DWORDS_16, r16, r17, r18, r19
#define ESM_REC_ARGS_14(d) d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], d[13]
#define ESM_REC_ARGS_16(d) ESM_REC_ARGS_14(d), d[14], d[15]
#define ESM_REC_ARGS_20(d) ESM_REC_ARGS_16(d), d[16], d[17], d[18], d[19]
#define ESM_REC_PARAMS(N) ESM_REC_PARAMS_##N
#define ESM_REC_DWORDS(N) {ESM_REC_DWORDS_##N}
#define ESM_REC_ARGS(N, d) ESM_REC_ARGS_##N(d)

// A kernel argument (the structs behind the record start at byte 4 N) read at an offset the compiler cannot see
// through, laundered by the caller: the scalar load stays where the source puts it.  Left alone, the epilogue's
// descriptor loads join the prologue's batch, where the first buffer_loads wait for them (s_waitcnt lgkmcnt(0)).
template <typename T>
__device__ __forceinline__ T kernarg_at(unsigned off) {
    typedef const char __attribute__((address_space(4))) * kptr;
    typedef const T __attribute__((address_space(4))) * tptr;
    return *(tptr)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + off);
}

}  // namespace conv
}  // namespace esm
