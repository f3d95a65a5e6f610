// The 2-D single-output ConvTranspose's first-load record (conv_c1.h convt_c1_batch_kernel): the 16 dwords a
// workgroup needs to find its tile and issue its staging loads, passed as the kernel's leading scalar arguments so
// that one scalar load of one 64-byte line brings all of them (after 4.14's lean record).  The by-value
// esm_conv_desc comes behind them (and behind 1 / up_f, divided on the host) and serves the epilogue only.
//
//   dword   field                                         dword   field
//   0-1     source base pointer                           10      Cin (8 bits) | XCD slab << 8
//   2-3     packed-weight pointer                         11      cin_pad / 16 | cout_pad / 32 << 16
//   4-5     source batch stride sb (64 bits)              12      grid x | grid y << 16     (slab order only)
//   6, 7    source strides sc, sh (0 for an axis of       13      workgroups of the grid    (slab order only)
//           one entry: the kernel would multiply it by 0) 14, 15  reciprocals of grid x, grid y (c1_magic)
//   8, 9    Hi, Wi
//
// Every descriptor convt_c1_ok accepts has a record (direct_ok bounds sc and sh, conv_check the padded extents), so
// there is no struct-argument twin.  The slab order divides by the grid extents with the reciprocals, which is exact
// while workgroups x extent <= 2^32; a grid past that (or past 16 bits in x or y) runs in dispatch order, which
// changes where a tile runs and nothing it computes.
#pragma once

#include "common.h"

namespace esm {
namespace conv {

constexpr int kC1RecDwords = 16;

struct C1Rec {
    const float* src;
    const float* w;
    long long sb;
    int sc, sh, Hi, Wi, Cin, cin_pad, cout_pad;
    bool slab;
    unsigned gx, gy, nwg, m_gx, m_gy;
};

// ceil(2^32 / d): __umulhi(n, m) == n / d while n * d <= 2^32; 0 stands for d = 1
inline unsigned c1_magic(unsigned d) {
    return d <= 1 ? 0u : static_cast<unsigned>(((1ull << 32) + d - 1) / d);
}

__host__ __device__ inline C1Rec c1_record_unpack(const unsigned (&d)[kC1RecDwords]) {
    C1Rec r;
    r.src = reinterpret_cast<const float*>(static_cast<unsigned long long>(d[1]) << 32 | d[0]);
    r.w = reinterpret_cast<const float*>(static_cast<unsigned long long>(d[3]) << 32 | d[2]);
    r.sb = static_cast<long long>(static_cast<unsigned long long>(d[5]) << 32 | d[4]);
    r.sc = static_cast<int>(d[6]), r.sh = static_cast<int>(d[7]);
    r.Hi = static_cast<int>(d[8]), r.Wi = static_cast<int>(d[9]);
    r.Cin = d[10] & 0xff, r.slab = (d[10] >> 8) & 1;
    r.cin_pad = 16 * (d[11] & 0xffff), r.cout_pad = 32 * (d[11] >> 16);
    r.gx = d[12] & 0xffff, r.gy = d[12] >> 16;
    r.nwg = d[13], r.m_gx = d[14], r.m_gy = d[15];
    return r;
}

// The record of a (checked, convt_c1_ok, 2-D) descriptor launched on `grid`.
inline void c1_record_pack(const esm_conv_desc& a, const dim3& grid, unsigned (&d)[kC1RecDwords]) {
    const esm_src& s = a.src[0];
    const unsigned long long sp = reinterpret_cast<unsigned long long>(s.ptr), wp = reinterpret_cast<unsigned long long>(a.w);
    const unsigned long long sb = static_cast<unsigned long long>(s.sb);
    const unsigned long long nwg = static_cast<unsigned long long>(grid.x) * grid.y * grid.z;
    const unsigned gmax = grid.x > grid.y ? grid.x : grid.y;
    const bool slab = (a.hint & ESM_HINT_XCD_SLAB) && grid.x <= 0xffffu && grid.y <= 0xffffu && nwg * gmax <= (1ull << 32);
    d[0] = static_cast<unsigned>(sp), d[1] = static_cast<unsigned>(sp >> 32);
    d[2] = static_cast<unsigned>(wp), d[3] = static_cast<unsigned>(wp >> 32);
    d[4] = static_cast<unsigned>(sb), d[5] = static_cast<unsigned>(sb >> 32);
    d[6] = a.Cin > 1 ? static_cast<unsigned>(s.sc) : 0u;
    d[7] = a.Hi > 1 ? static_cast<unsigned>(s.sh) : 0u;
    d[8] = static_cast<unsigned>(a.Hi), d[9] = static_cast<unsigned>(a.Wi);
    d[10] = static_cast<unsigned>(a.Cin) | (slab ? 1u << 8 : 0u);
    d[11] = static_cast<unsigned>(a.cin_pad / 16) | static_cast<unsigned>(a.cout_pad / 32) << 16;
    d[12] = slab ? grid.x | grid.y << 16 : 0u;
    d[13] = slab ? static_cast<unsigned>(nwg) : 0u;
    d[14] = slab ? c1_magic(grid.x) : 0u;
    d[15] = slab ? c1_magic(grid.y) : 0u;
}

#define ESM_C1_REC_PARAMS                                                                                       \
    unsigned r0, unsigned r1, unsigned r2, unsigned r3, unsigned r4, unsigned r5, unsigned r6, unsigned r7,     \
        unsigned r8, unsigned r9, unsigned r10, unsigned r11, unsigned r12, unsigned r13, unsigned r14, unsigned r15
#define ESM_C1_REC_UNPACK c1_record_unpack({r0, r1, r2, r3, r4, r5, r6, r7, r8, r9, r10, r11, r12, r13, r14, r15})
#define ESM_C1_REC_ARGS(d) \
    d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7], d[8], d[9], d[10], d[11], d[12], d[13], d[14], d[15]

#ifdef __HIPCC__
// xcd_block (common.h) from the record: the same bijection, the grid extents and their reciprocals from the leading
// arguments instead of the dispatch packet, so nothing is loaded or divided on the way to the tile's coordinates
__device__ __forceinline__ Blk3 c1_block(const C1Rec& r) {
    if (!r.slab) return {static_cast<int>(blockIdx.x), static_cast<int>(blockIdx.y), static_cast<int>(blockIdx.z)};
    const unsigned orig = blockIdx.x + r.gx * (blockIdx.y + r.gy * blockIdx.z);
    const unsigned q = r.nwg / 8, rem = r.nwg % 8, xcd = orig % 8;
    const unsigned wg = (xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q) + orig / 8;
    const unsigned t = r.m_gx ? __umulhi(wg, r.m_gx) : wg;
    const unsigned z = r.m_gy ? __umulhi(t, r.m_gy) : t;
    return {static_cast<int>(wg - t * r.gx), static_cast<int>(t - z * r.gy), static_cast<int>(z)};
}

// A kernel argument read at a byte offset the compiler cannot see through (laundered by the caller): the scalar load
// stays where the source puts it instead of joining the prologue's batch (conv_small.hip kernarg_at)
template <typename T>
__device__ __forceinline__ T c1_kernarg(unsigned off) {
    typedef const char __attribute__((address_space(4))) * kptr;
    typedef const T __attribute__((address_space(4))) * tptr;
    return *(tptr)((kptr)__builtin_amdgcn_kernarg_segment_ptr() + off);
}
#endif

}  // namespace conv
}  // namespace esm
