// The LDS pair's staging record (conv_pair2.hip): the 20 dwords a workgroup needs to issue every staging load -- the
// input window, both weight slabs, the four BN vectors -- passed as the kernel's leading scalar arguments, so that
// the first vector load waits for one scalar batch (conv_lean_rec.h is the lean form's).  The two
// by-value esm_conv_desc come behind it and serve the output side only.
//
//   dword   field                                      dword   field
//   0-1     source 0 base pointer                      12-13   source 1 base pointer    (REGRESS: a.out)
//   2-3     convA packed-weight pointer                14-15   source 2 base pointer
//   4-5     convB packed-weight pointer                16      source 1 batch stride    (REGRESS: a.ob)
//   6       source 0 batch stride                      17      source 2 batch stride    (REGRESS: a.oh)
//   7, 8    channel / row stride of every source       18      C0 | (C0 + C1) << 8
//   9       Wi | Hi << 16                              19      0
//   10      Cin (7 bits) | a.ph (3) << 7 | b.ph (2) << 10 | b.Cout (5) << 12 | nsrc (2) << 17 | XCD slab << 19
//   11      REGRESS: D, the cost planes of source 0 (their stride is dword 7)
//
// Strides are elements, each in [0, 2^31); the sources share their channel and row strides (maps of one extent
// do, unless they are views of different parents).  The packed weights follow engine.pack_weight: cin_pad = Cin
// rounded up to 16 (16 for convB), cout_pad = 32; a slab is then copied to LDS in 16-byte pieces, the 16 couts of a
// (tap, cin) row being 64 contiguous bytes.  Rows past Cin and convB's couts past Cout are masked, not trusted to be
// zero.  The BN constants are read through the weight pointers: [scale | shift], 32 floats each, directly behind the
// packed weights (engine.pack_conv lays them out so).  pair2_record_pack refuses every pair the record cannot
// describe, and the launcher then runs the struct-argument kernel.
#pragma once

#include "kernarg_rec.h"

namespace esm {
namespace conv {

constexpr int kPair2RecDwords = 20;
constexpr int kPair2RecFields = 24;  // P2Rec's members, in order (esm_pair2_record_pack)

struct P2Rec {
    const float* src0;
    const float* wa;
    const float* wb;
    int sb0, sc, sh;
    int Wi, Hi;
    int Cin, pa, pb, CoutB, nsrc;
    bool xcd;
    int D;
    const float* src1;
    const float* src2;
    int sb1, sb2;
    int C0, C01;
    // REGRESS (one source): the stored map, in the second source's dwords
    float* out;
    int ob, oh;
};

// the limits of the packed fields
constexpr int kPair2MaxExtent = 0xffff;  // Wi, Hi, D
constexpr int kPair2MaxCin = 64;
constexpr int kPair2MaxPadA = 7, kPair2MaxPadB = 3;
constexpr int kPair2CoutPad = 32;        // both convs: 16 couts padded as engine.pack_weight pads them
constexpr unsigned kPair2MaxSpan = 0x40000000u;  // bytes of one source's batch item: below the kernels' kOOB mark

__host__ __device__ inline P2Rec pair2_record_unpack(const unsigned (&d)[kPair2RecDwords]) {
    P2Rec r;
    r.src0 = ptr_join(d[0], d[1]), r.wa = ptr_join(d[2], d[3]), r.wb = ptr_join(d[4], d[5]);
    r.sb0 = static_cast<int>(d[6]), r.sc = static_cast<int>(d[7]), r.sh = static_cast<int>(d[8]);
    r.Wi = d[9] & 0xffff, r.Hi = d[9] >> 16;
    r.Cin = d[10] & 0x7f, r.pa = (d[10] >> 7) & 7, r.pb = (d[10] >> 10) & 3, r.CoutB = (d[10] >> 12) & 0x1f;
    r.nsrc = (d[10] >> 17) & 3, r.xcd = (d[10] >> 19) & 1;
    r.D = static_cast<int>(d[11]);
    r.src1 = ptr_join(d[12], d[13]), r.src2 = ptr_join(d[14], d[15]);
    r.sb1 = static_cast<int>(d[16]), r.sb2 = static_cast<int>(d[17]);
    r.C0 = d[18] & 0xff, r.C01 = (d[18] >> 8) & 0xff;
    r.out = const_cast<float*>(r.src1), r.ob = r.sb1, r.oh = r.sb2;
    return r;
}

// The record of a pair pair2_lds_ok accepted; false: the record cannot describe this pair.
inline bool pair2_record_pack(const esm_conv_desc& a, const esm_conv_desc& b, unsigned (&d)[kPair2RecDwords]) {
    const bool reg = (a.hint & ESM_HINT_PAIR_REGRESS) != 0;
    if (a.nsrc < 1 || a.nsrc > 3 || (reg && a.nsrc != 1)) return false;
    const esm_src& s0 = a.src[0];
    int csum = 0;
    for (int i = 0; i < a.nsrc; ++i) {
        const esm_src& s = a.src[i];
        if (!s.ptr || s.C < 1) return false;
        if (!strides_fit({s.sb, s.sc, s.sh})) return false;
        if (s.sc != s0.sc || s.sh != s0.sh) return false;
        const long long span = 4 * ((s.C - 1) * s.sc + (a.Hi - 1) * s.sh + a.Wi);
        if (!reg && span >= static_cast<long long>(kPair2MaxSpan)) return false;
        csum += s.C;
    }
    for (const int e : {a.Wi, a.Hi})
        if (e < 1 || e > kPair2MaxExtent) return false;
    if (a.Cin < 1 || a.Cin > kPair2MaxCin || (reg ? a.Cin != 1 || s0.C > kPair2MaxExtent : csum != a.Cin)) return false;
    if (a.ph < 0 || a.ph > kPair2MaxPadA || b.ph < 0 || b.ph > kPair2MaxPadB || b.Cout < 1 || b.Cout > 16) return false;
    // the packing of engine.pack_weight / pack_conv: [taps][cin_pad][32] | scale | shift, 16-byte aligned
    if (a.cin_pad != ((a.Cin + 15) & ~15) || a.cout_pad != kPair2CoutPad || b.cin_pad != 16 || b.cout_pad != kPair2CoutPad)
        return false;
    for (const esm_conv_desc* c : {&a, &b}) {
        const long long nw = static_cast<long long>(c->kh) * c->kw * c->cin_pad * c->cout_pad;
        if ((reinterpret_cast<uintptr_t>(c->w) & 15) || !bn_behind_weights(*c, nw, false)) return false;
    }
    if (reg && (!a.out || !strides_fit({a.ob, a.oh}))) return false;

    const esm_src& s1 = a.src[a.nsrc > 1 ? 1 : 0];
    const esm_src& s2 = a.src[a.nsrc > 2 ? 2 : 0];
    d[0] = ptr_lo(s0.ptr), d[1] = ptr_hi(s0.ptr), d[2] = ptr_lo(a.w), d[3] = ptr_hi(a.w), d[4] = ptr_lo(b.w), d[5] = ptr_hi(b.w);
    d[6] = static_cast<unsigned>(s0.sb), d[7] = static_cast<unsigned>(s0.sc), d[8] = static_cast<unsigned>(s0.sh);
    d[9] = static_cast<unsigned>(a.Wi) | static_cast<unsigned>(a.Hi) << 16;
    d[10] = static_cast<unsigned>(a.Cin) | static_cast<unsigned>(a.ph) << 7 | static_cast<unsigned>(b.ph) << 10 |
            static_cast<unsigned>(b.Cout) << 12 | static_cast<unsigned>(a.nsrc) << 17 |
            ((a.hint & ESM_HINT_XCD_SLAB) ? 1u << 19 : 0u);
    d[11] = reg ? static_cast<unsigned>(s0.C) : 0u;
    if (reg) {
        d[12] = ptr_lo(a.out), d[13] = ptr_hi(a.out), d[14] = d[15] = 0;
        d[16] = static_cast<unsigned>(a.ob), d[17] = static_cast<unsigned>(a.oh);
        d[18] = 1u | 1u << 8;
    } else {
        d[12] = ptr_lo(s1.ptr), d[13] = ptr_hi(s1.ptr), d[14] = ptr_lo(s2.ptr), d[15] = ptr_hi(s2.ptr);
        d[16] = static_cast<unsigned>(s1.sb), d[17] = static_cast<unsigned>(s2.sb);
        const int c0 = s0.C, c01 = c0 + (a.nsrc > 1 ? s1.C : 0);
        d[18] = static_cast<unsigned>(c0) | static_cast<unsigned>(c01) << 8;
    }
    d[19] = 0;
    return true;
}

}  // namespace conv
}  // namespace esm
