// The lean form's first-load record (conv_small.hip): the 14 dwords a wave needs to issue its first batch of
// loads for a single-source layer, passed as the kernel's leading scalar arguments so that one scalar load of
// one 64-byte line brings all of them.  The by-value esm_conv_desc comes behind them and serves the
// output side only.
//
//   dword   field
//   0-1     source base pointer                 8, 9   the grid reciprocals m_ds, m_b (magic_for)
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

#include "common.h"

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

inline unsigned lean_magic(int d) {
    return d <= 1 ? 0u : static_cast<unsigned>(((1ull << 32) + static_cast<unsigned long long>(d) - 1) / d);
}

__host__ __device__ inline LeanRec lean_record_unpack(const unsigned (&d)[kLeanRecDwords]) {
    LeanRec r;
    r.src = reinterpret_cast<const float*>(static_cast<unsigned long long>(d[1]) << 32 | d[0]);
    r.w = reinterpret_cast<const float*>(static_cast<unsigned long long>(d[3]) << 32 | d[2]);
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
    const bool d3 = is3d(a);
    const int Ws = a.transposed ? a.Wi : a.Wo;
    const int Ds = d3 ? (a.transposed ? a.Di : a.Do) : 1;
    const esm_src& s = a.src[0];
    if (a.nsrc != 1 || s.C != a.Cin) return false;  // a second source: its groups are some wave's first loads
    for (const int64_t st : {s.sb, s.sc, s.sd, s.sh})
        if (st < 0 || st >= (1ll << 31)) return false;
    for (const int e : {a.Wi, a.Hi, a.Di, Ws, Ds, a.B})
        if (e < 0 || e > kLeanMaxExtent) return false;
    if (a.Cin < 1 || a.Cin > kLeanMaxCin || a.cin_pad != ((a.Cin + 15) & ~15)) return false;
    if (a.cout_pad < 32 || a.cout_pad % 32 || a.cout_pad > kLeanMaxCoutPad) return false;
    for (const int p : {a.pd, a.ph, a.pw})
        if (p < 0 || p > kLeanMaxPad) return false;
    // BN constants behind the packed weights: [taps][cin_pad][cout_pad] (x parity classes) | scale | shift
    const int kdt = d3 ? a.kd : 1;
    const long long nw = static_cast<long long>(kdt) * a.kh * a.kw * a.cin_pad * a.cout_pad;  // transposed: 4^nd = cls x taps
    if (!a.w || !a.shift || a.shift != a.w + nw + a.cout_pad) return false;
    if (a.scale && a.scale != a.w + nw) return false;

    const unsigned long long sp = reinterpret_cast<unsigned long long>(s.ptr), wp = reinterpret_cast<unsigned long long>(a.w);
    d[0] = static_cast<unsigned>(sp), d[1] = static_cast<unsigned>(sp >> 32);
    d[2] = static_cast<unsigned>(wp), d[3] = static_cast<unsigned>(wp >> 32);
    d[4] = static_cast<unsigned>(s.sb), d[5] = static_cast<unsigned>(s.sc);
    d[6] = static_cast<unsigned>(s.sd), d[7] = static_cast<unsigned>(s.sh);
    d[8] = lean_magic(Ds), d[9] = lean_magic(a.B);
    d[10] = static_cast<unsigned>(a.Wi) | static_cast<unsigned>(a.Hi) << 16;
    d[11] = static_cast<unsigned>(a.Di) | static_cast<unsigned>(Ws) << 16;
    d[12] = static_cast<unsigned>(Ds) | static_cast<unsigned>(a.B) << 16;
    d[13] = static_cast<unsigned>(a.Cin) | static_cast<unsigned>(a.cout_pad / 32) << 10 | static_cast<unsigned>(a.pd) << 14 |
            static_cast<unsigned>(a.ph) << 17 | static_cast<unsigned>(a.pw) << 20 |
            ((a.hint & ESM_HINT_XCD_SLAB) ? 1u << 23 : 0u) | (a.scale ? 1u << 24 : 0u);
    return true;
}

}  // namespace conv
}  // namespace esm
