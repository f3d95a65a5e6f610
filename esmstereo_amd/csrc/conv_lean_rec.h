// The lean form's first-load record (conv_small.hip): the 14 dwords a wave needs to issue its first batch of
// loads for a single-source layer, passed as the kernel's leading scalar arguments so that one scalar load of
// one 64-byte line brings all of them.  The by-value esm_conv_desc comes behind them and serves the
// output side only.
//
//   dword   field
//   0-1     source base pointer                 8, 9   the grid reciprocals m_ds, m_b (magic_u32)
//   2-3     packed-weight pointer               10     Wi | Hi << 16
//   4-7     source strides sb, sc, sd, sh       11     Di | Ws << 16          (Ws, Ds: the sub-grid the
//           (elements, each in [0, 2^31))       12     Ds | B << 16            workgroups tile)
//                                               13     Cin (10 bits) | cout_pad / 32 (4) << 10 | pd (3) << 14 |
//                                                      ph (3) << 17 | pw (3) << 20 | XCD slab << 23 | scale << 24
//
// cin_pad is Cin rounded up to 16.  The BN constants are read through the weight pointer: [scale | shift], cout_pad
// floats each, directly behind the packed weights (engine.pack_conv lays them out so); `scale` (bit 24) says whether
// the descriptor has a scale at all.  lean_record_pack refuses every layer the record cannot describe, and the
// launcher then runs the struct-argument kernel.
#pragma once

#include "kernarg_rec.h"

namespace esm {
namespace conv {

constexpr int kLeanRecDwords = 14;

struct LeanRec {
    const float* src;
    const float* w;
    int sb, sc, sd, sh;
    unsigned m_ds, m_b;
    int Wi, Hi, Di, Ws, Ds, B;
    int Cin, cout_pad, pd, ph, pw;
    bool xcd, has_scale;
};

// the limits of the packed fields
constexpr int kLeanMaxExtent = 0xffff;  // Wi, Hi, Di, Ws, Ds, B
constexpr int kLeanMaxCin = 0x3ff;
constexpr int kLeanMaxCoutPad = 15 * 32;
constexpr int kLeanMaxPad = 7;

// The sub-grid the workgroups tile and the reciprocals of the z split: the record's, and the struct-argument kernels'
struct LeanGrid {
    int Ws, Ds;
    unsigned m_ds, m_b;
};
inline LeanGrid lean_grid(const esm_conv_desc& a) {
    const int Ds = is3d(a) ? (a.transposed ? a.Di : a.Do) : 1;
    return {a.transposed ? a.Wi : a.Wo, Ds, magic_u32(Ds), magic_u32(a.B)};
}

__host__ __device__ inline LeanRec lean_record_unpack(const unsigned (&d)[kLeanRecDwords]) {
    LeanRec r;
    r.src = ptr_join(d[0], d[1]), r.w = ptr_join(d[2], d[3]);
    r.sb = static_cast<int>(d[4]), r.sc = static_cast<int>(d[5]), r.sd = static_cast<int>(d[6]), r.sh = static_cast<int>(d[7]);
    r.m_ds = d[8], r.m_b = d[9];
    r.Wi = d[10] & 0xffff, r.Hi = d[10] >> 16;
    r.Di = d[11] & 0xffff, r.Ws = d[11] >> 16;
    r.Ds = d[12] & 0xffff, r.B = d[12] >> 16;
    r.Cin = d[13] & 0x3ff, r.cout_pad = 32 * ((d[13] >> 10) & 0xf);
    r.pd = (d[13] >> 14) & 7, r.ph = (d[13] >> 17) & 7, r.pw = (d[13] >> 20) & 7;
    r.xcd = (d[13] >> 23) & 1, r.has_scale = (d[13] >> 24) & 1;
    return r;
}

// The record of a (checked, small_ok) descriptor; false: the record cannot describe this layer.
inline bool lean_record_pack(const esm_conv_desc& a, unsigned (&d)[kLeanRecDwords]) {
    const LeanGrid g = lean_grid(a);
    const esm_src& s = a.src[0];
    if (a.nsrc != 1 || s.C != a.Cin) return false;  // a second source: its groups are some wave's first loads
    if (!strides_fit({s.sb, s.sc, s.sd, s.sh})) return false;
    for (const int e : {a.Wi, a.Hi, a.Di, g.Ws, g.Ds, a.B})
        if (e < 0 || e > kLeanMaxExtent) return false;
    if (a.Cin < 1 || a.Cin > kLeanMaxCin || a.cin_pad != ((a.Cin + 15) & ~15)) return false;
    if (a.cout_pad < 32 || a.cout_pad % 32 || a.cout_pad > kLeanMaxCoutPad) return false;
    for (const int p : {a.pd, a.ph, a.pw})
        if (p < 0 || p > kLeanMaxPad) return false;
    const int kdt = is3d(a) ? a.kd : 1;
    const long long nw = static_cast<long long>(kdt) * a.kh * a.kw * a.cin_pad * a.cout_pad;  // transposed: 4^nd = cls x taps
    if (!bn_behind_weights(a, nw, true)) return false;

    d[0] = ptr_lo(s.ptr), d[1] = ptr_hi(s.ptr), d[2] = ptr_lo(a.w), d[3] = ptr_hi(a.w);
    d[4] = static_cast<unsigned>(s.sb), d[5] = static_cast<unsigned>(s.sc);
    d[6] = static_cast<unsigned>(s.sd), d[7] = static_cast<unsigned>(s.sh);
    d[8] = g.m_ds, d[9] = g.m_b;
    d[10] = static_cast<unsigned>(a.Wi) | static_cast<unsigned>(a.Hi) << 16;
    d[11] = static_cast<unsigned>(a.Di) | static_cast<unsigned>(g.Ws) << 16;
    d[12] = static_cast<unsigned>(g.Ds) | static_cast<unsigned>(a.B) << 16;
    d[13] = static_cast<unsigned>(a.Cin) | static_cast<unsigned>(a.cout_pad / 32) << 10 | static_cast<unsigned>(a.pd) << 14 |
            static_cast<unsigned>(a.ph) << 17 | static_cast<unsigned>(a.pw) << 20 |
            ((a.hint & ESM_HINT_XCD_SLAB) ? 1u << 23 : 0u) | (a.scale ? 1u << 24 : 0u);
    return true;
}

}  // namespace conv
}  // namespace esm
