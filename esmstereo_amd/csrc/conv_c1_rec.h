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
//           one entry: the kernel would multiply it by 0) 14, 15  reciprocals of grid x, grid y (magic_u32)
//   8, 9    Hi, Wi
//
// Every descriptor convt_c1_ok accepts has a record (direct_ok bounds sc and sh, conv_check the padded extents), so
// there is no struct-argument twin.  The slab order divides by the grid extents with the reciprocals, which is exact
// while workgroups x extent <= 2^32; a grid past that (or past 16 bits in x or y) runs in dispatch order, which
// changes where a tile runs and nothing it computes.
#pragma once

#include "kernarg_rec.h"

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

__host__ __device__ inline C1Rec c1_record_unpack(const unsigned (&d)[kC1RecDwords]) {
    C1Rec r;
    r.src = ptr_join(d[0], d[1]), r.w = ptr_join(d[2], d[3]);
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
    const unsigned long long sb = static_cast<unsigned long long>(s.sb);
    const unsigned long long nwg = static_cast<unsigned long long>(grid.x) * grid.y * grid.z;
    const unsigned gmax = grid.x > grid.y ? grid.x : grid.y;
    const bool slab = (a.hint & ESM_HINT_XCD_SLAB) && grid.x <= 0xffffu && grid.y <= 0xffffu && nwg * gmax <= (1ull << 32);
    d[0] = ptr_lo(s.ptr), d[1] = ptr_hi(s.ptr), d[2] = ptr_lo(a.w), d[3] = ptr_hi(a.w);
    d[4] = static_cast<unsigned>(sb), d[5] = static_cast<unsigned>(sb >> 32);
    d[6] = a.Cin > 1 ? static_cast<unsigned>(s.sc) : 0u;
    d[7] = a.Hi > 1 ? static_cast<unsigned>(s.sh) : 0u;
    d[8] = static_cast<unsigned>(a.Hi), d[9] = static_cast<unsigned>(a.Wi);
    d[10] = static_cast<unsigned>(a.Cin) | (slab ? 1u << 8 : 0u);
    d[11] = static_cast<unsigned>(a.cin_pad / 16) | static_cast<unsigned>(a.cout_pad / 32) << 16;
    d[12] = slab ? grid.x | grid.y << 16 : 0u;
    d[13] = slab ? static_cast<unsigned>(nwg) : 0u;
    d[14] = slab ? magic_u32(grid.x) : 0u;
    d[15] = slab ? magic_u32(grid.y) : 0u;
}

// xcd_block (common.h) from the record: the same bijection, the grid extents and their reciprocals from the leading
// arguments instead of the dispatch packet, so nothing is loaded or divided on the way to the tile's coordinates
__host__ __device__ __forceinline__ Blk3 c1_tile(const C1Rec& r, unsigned bx, unsigned by, unsigned bz) {
    if (!r.slab) return {static_cast<int>(bx), static_cast<int>(by), static_cast<int>(bz)};
    const unsigned wg = xcd_slab_wg(bx + r.gx * (by + r.gy * bz), r.nwg);
    const unsigned t = magic_div(wg, r.m_gx), z = magic_div(t, r.m_gy);
    return {static_cast<int>(wg - t * r.gx), static_cast<int>(t - z * r.gy), static_cast<int>(z)};
}
__device__ __forceinline__ Blk3 c1_block(const C1Rec& r) { return c1_tile(r, blockIdx.x, blockIdx.y, blockIdx.z); }

}  // namespace conv
}  // namespace esm
