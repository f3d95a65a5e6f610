// Two consecutive 2-D BasicConvs in one launch, both through LDS (halo recomputation):
//   y = actB(BN_B(convB(actA(BN_A(convA(cat(sources)))))))
// convA: k 1/3/5, stride 1/2, any padding, <= 48 input channels (64 for 1x1) over up to 3 sources, 16 outputs;
// convB: k 1/3, stride 1, 16 inputs, <= 16 outputs.  The pairs of the ESM upsampler stages and the
// refinement hourglasses (models/ESMStereo.py:185-239, 247-259 and twins): dm<t>.0 -> dm<t>.1,
// dm<t>.2 -> dm<t>.3, spx_<t>.0 -> spx_<t>.1, conv2.0 -> conv2.1, conv3.0 -> conv3.1.
//
// Why: on the 1/16..1/4-resolution maps of ESMStereo-S each of these convs is a latency floor
// (~4.5 us per launch, ~2 us of it serial memory round trips: profiles/r02_pmc_sq_ops_SK_b.txt).
// Here one round trip stages everything a workgroup needs -- the input window of its tile (+ the
// halo both convs need), both weight slabs, both BN affines -- into LDS; convA runs on the tile +
// convB's halo into LDS (zero outside A's extent: convB's zero padding), convB runs from LDS and
// stores.  The intermediate map never touches memory, and the launch between the two is gone.
//
// MFMA mapping (v_mfma_f32_16x16x4_f32): M = 16 output channels, N = 16 pixels of one tile row,
// k = 4 input channels.  A workgroup owns TH output rows x (16 - KB + 1) output columns; convA
// computes TH + KB - 1 rows x 16 columns.  4 waves: rows round-robin in both phases.
//
// Two staging prologues in front of the same MFMA phases and epilogues (the same bits): behind the
// staging record (pair2_rec_kernel, P2Stage; conv_pair2_rec.h) for every pair the record describes, and with struct
// arguments (pair2_kernel) for the others and under ESM_HINT_PAIR_NO_RECORD.
#include <cstddef>

#include "conv_direct.h"
#include "conv_pair2_rec.h"

namespace esm {
namespace conv {
namespace {

constexpr int kP2Threads = 256;
// PAIR_REGRESS in convA's hint: its single input channel is disparity_regression of the cost volume in src[0]
// (src[0].C = D planes), also stored to a.out (see pair2_lds_ok)

// disparity_regression at one pixel, as regression.hip dispreg_kernel: products rounded, then summed in
// d order (torch.sum(x * arange)): the same bits as the separate launch
__device__ __forceinline__ float regress_px(const float* __restrict__ cp, int D, int sc) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int d0 = 0; d0 < D; d0 += 16) {
        float v[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) v[k] = d0 + k < D ? cp[(d0 + k) * sc] : 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (d0 + k < D) acc = acc + v[k] * static_cast<float>(d0 + k);
    }
    return acc;
}

template <int KA, int SA, int KB, int TH>
struct P2Geo {
    static constexpr int NA = TH + KB - 1;        // convA rows per tile
    static constexpr int IR = (NA - 1) * SA + KA;   // staged input rows
    static constexpr int IC = 15 * SA + KA;         // staged input columns
    static constexpr int ICP = IC;
    static constexpr int ICS0 = IR * ICP;
    static constexpr int ICS = ICS0 + ((16 - ICS0 % 64) + 64) % 64;  // channel stride = 16 (mod 64)
    static constexpr int AR = 18;                                   // convA row in LDS (16 + dx overrun)
    static constexpr int ACS0 = NA * AR;
    static constexpr int ACS = ACS0 + ((16 - ACS0 % 64) + 64) % 64;
};

// what the two convs' epilogues read of the descriptors
struct P2Out {
    float* out;
    long long ob;
    int oc, oh, Cout, Ho, Wo, aHo, aWo;
};

typedef unsigned p2_u32x4 __attribute__((ext_vector_type(4)));
static_assert(kPair2MaxSpan == kOOB, "the record admits source spans below the out-of-range mark");

// The staging prologue behind the record (conv_pair2_rec.h): every load of a thread in flight together (load), then
// the LDS stores (store).  The struct-argument prologue spent most of its instructions on per-element index
// arithmetic between its loads (e % IC, (e / IC) % IR, a three-way source select, the tap / c / co split of every
// weight); here, as conv_c1.h C1Stage:
//   window   a thread's slots in one 4-channel group [4][IR][IC] (element tid + 256 k) are fixed once: their buffer
//            offset at group 0 (kOOB outside the map) and their LDS index.  Group g is then one buffer load per slot,
//            its source (wave-uniform: the sources split at 4-channel boundaries) in the descriptor and its channel
//            offset in soffset; zeros outside the map and past Cin come from the range check;
//   weights  16-byte pieces: the 16 couts of a (tap, cin) row are contiguous in the packed layout and in LDS;
//   BN       through the weight descriptors, [scale | shift] behind the packed weights.
// REG keeps regress_px and the owner tile's store; its pixel slots are [IR][IC] (channel 0), channels 1-3 zero.
template <int KA, int SA, int KB, int TH, int CINMAX, bool REG, bool MS>
struct P2Stage {
    using G = P2Geo<KA, SA, KB, TH>;
    static constexpr int IR = G::IR, IC = G::IC, ICP = G::ICP, ICS = G::ICS;
    static constexpr int TA = KA * KA, TB = KB * KB, VB = 16 - KB + 1;
    static constexpr int NPX = IR * IC;                                       // pixels of the window
    static constexpr int NCH = 4 * NPX;                                       // elements of one 4-channel group
    static constexpr int XR = ((REG ? NPX : NCH) + kP2Threads - 1) / kP2Threads;  // slots per thread
    static constexpr int NG = REG ? 1 : CINMAX / 4;
    static constexpr int NA4 = TA * CINMAX * 4, PA4 = (NA4 + kP2Threads - 1) / kP2Threads;  // 16-byte pieces of wa
    static constexpr int NB4 = TB * 64, PB4 = (NB4 + kP2Threads - 1) / kP2Threads;          // ... of wb
    static_assert(!REG || CINMAX == 4, "the regressed map is the pair's only input channel");
    static_assert(!MS || (!REG && CINMAX >= 8), "several sources: at least two 4-channel groups");
    static_assert(CINMAX % 4 == 0 && ICS % 4 == 0, "16-byte aligned weight slabs in LDS");
    int sidx[XR];
    float vi[NG][XR];
    p2_u32x4 vwa[PA4], vwb[PB4];
    float vep;

    __device__ __forceinline__ void load(const P2Rec& r, int tid, const Blk3& bk, int yi0, int xi0) {
        const int b = bk.z, cin = r.Cin;
        if constexpr (!REG) {
            unsigned voff[XR];
            int crel[XR];
#pragma unroll
            for (int k = 0; k < XR; ++k) {
                const int i = tid + k * kP2Threads;
                const int q = i % IC, rw = (i / IC) % IR, cr = i / (IC * IR);
                const int yi = yi0 + rw, xi = xi0 + q;
                const bool ok = i < NCH && yi >= 0 && yi < r.Hi && xi >= 0 && xi < r.Wi;
                voff[k] = ok ? 4u * static_cast<unsigned>(cr * r.sc + yi * r.sh + xi) : kOOB;
                crel[k] = cr;
                sidx[k] = cr * ICS + rw * ICP + q;
            }
            // (the record's members as values: a select between two members' addresses keeps the struct in scratch)
            const float *p0 = r.src0, *p1 = r.src1, *p2 = r.src2;
            const int sb0 = r.sb0, sb1 = r.sb1, sb2 = r.sb2, C0 = r.C0, C01 = r.C01;
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                // the group's source (MS; else source 0, one descriptor for every group); a group past Cin reads
                // nothing: its lanes are out of range, and so is every offset of an empty descriptor
                const int c0 = 4 * g, rem = cin - c0;
                const bool s1 = MS && c0 >= C0, s2 = MS && c0 >= C01;
                const float* sp = s2 ? +p2 : (s1 ? +p1 : +p0);
                const int sb = s2 ? +sb2 : (s1 ? +sb1 : +sb0);
                const int lo = s2 ? +C01 : (s1 ? +C0 : 0);
                const int cs = !MS ? cin : (s2 ? cin - C01 : (s1 ? C01 - C0 : C0));
                const bool live = rem > 0 && cs > 0;
                const int span = (!MS || live) ? 4 * ((cs - 1) * r.sc + (r.Hi - 1) * r.sh + r.Wi) : 0;
                const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float*>(sp + static_cast<long long>(b) * sb), static_cast<short>(0), span, 0x00020000);
                const int soff = live ? 4 * (c0 - lo) * r.sc : 0;
#pragma unroll
                for (int k = 0; k < XR; ++k) vi[g][k] = buf_load_s(rs, crel[k] < rem ? voff[k] : kOOB, soff);
            }
        }
        const int cin_pad = (cin + 15) & ~15;
        const int nwa = TA * cin_pad * kPair2CoutPad, nwb = TB * 16 * kPair2CoutPad;  // floats ahead of [scale | shift]
        const __amdgpu_buffer_rsrc_t rsa = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(r.wa), static_cast<short>(0), 4 * (nwa + 2 * kPair2CoutPad), 0x00020000);
        const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(r.wb), static_cast<short>(0), 4 * (nwb + 2 * kPair2CoutPad), 0x00020000);
        const int q4 = tid & 3;
#pragma unroll
        for (int i = 0; i < PA4; ++i) {  // piece e4 = row (tap, c) x couts 4 q4 .. 4 q4 + 3
            const int row = (tid >> 2) + i * (kP2Threads / 4);
            const int tap = row / CINMAX, c = row % CINMAX;
            const bool ok = row < TA * CINMAX && c < cin;
            vwa[i] = __builtin_amdgcn_raw_buffer_load_b128(
                rsa, static_cast<int>(ok ? 16u * static_cast<unsigned>((tap * cin_pad + c) * (kPair2CoutPad / 4) + q4) : kOOB), 0, 0);
        }
#pragma unroll
        for (int i = 0; i < PB4; ++i) {  // rows (tap, c) of 16 channels: row = tap * 16 + c in both layouts
            const int row = (tid >> 2) + i * (kP2Threads / 4);
            const p2_u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(
                rsb, static_cast<int>(row < TB * 16 ? 16u * static_cast<unsigned>(row * (kPair2CoutPad / 4) + q4) : kOOB), 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) vwb[i][j] = 4 * q4 + j < r.CoutB ? v[j] : 0u;
        }
        vep = 0.f;
        if (tid < 64) {  // scaleA, shiftA, scaleB, shiftB
            const int k = tid >> 4, c = tid & 15;
            const unsigned o = 4u * static_cast<unsigned>((k < 2 ? nwa : nwb) + (k & 1) * kPair2CoutPad + c);
            const float va = buf_load_s(rsa, k < 2 ? o : kOOB, 0), vb = buf_load_s(rsb, k < 2 ? kOOB : o, 0);
            const bool ok = k < 2 || c < r.CoutB;
            vep = ok ? (k < 2 ? va : vb) : ((k & 1) ? 0.f : 1.f);
        }
        if constexpr (REG) {
            // after the weight loads, as in the struct-argument prologue (see there, and for the owner tile)
            const float* sp0 = r.src0 + static_cast<long long>(b) * r.sb0;
            const int yb0 = bk.y * TH, xb0 = bk.x * VB;
#pragma unroll
            for (int k = 0; k < XR; ++k) {
                const int e = tid + k * kP2Threads;
                const int q = e % IC, rw = e / IC;
                const int yi = yi0 + rw, xi = xi0 + q;
                sidx[k] = rw * ICP + q;
                vi[0][k] = 0.f;
                if (e < NPX && yi >= 0 && yi < r.Hi && xi >= 0 && xi < r.Wi) {
                    const float v = regress_px(sp0 + yi * r.sh + xi, r.D, r.sc);
                    vi[0][k] = v;
                    const bool own_y = (bk.y == 0 || yi >= yb0) && (bk.y == static_cast<int>(gridDim.y) - 1 || yi < yb0 + TH);
                    const bool own_x = (bk.x == 0 || xi >= xb0) && (bk.x == static_cast<int>(gridDim.x) - 1 || xi < xb0 + VB);
                    if (own_y && own_x)
                        r.out[static_cast<long long>(b) * r.ob + static_cast<long long>(yi) * r.oh + xi] = v;
                }
            }
        }
    }

    __device__ __forceinline__ void store(float* in, float* wa, float* wb, float* ep, int tid) const {
#pragma unroll
        for (int g = 0; g < NG; ++g)
#pragma unroll
            for (int k = 0; k < XR; ++k) {
                if ((k + 1) * kP2Threads > (REG ? NPX : NCH) && tid + k * kP2Threads >= (REG ? NPX : NCH)) continue;
                in[4 * g * ICS + sidx[k]] = vi[g][k];
                if constexpr (REG) in[ICS + sidx[k]] = in[2 * ICS + sidx[k]] = in[3 * ICS + sidx[k]] = 0.f;
            }
#pragma unroll
        for (int i = 0; i < PA4; ++i)
            if ((i + 1) * kP2Threads <= NA4 || tid + i * kP2Threads < NA4)
                reinterpret_cast<p2_u32x4*>(wa)[tid + i * kP2Threads] = vwa[i];
#pragma unroll
        for (int i = 0; i < PB4; ++i)
            if ((i + 1) * kP2Threads <= NB4 || tid + i * kP2Threads < NB4)
                reinterpret_cast<p2_u32x4*>(wb)[tid + i * kP2Threads] = vwb[i];
        if (tid < 64) ep[tid] = vep;
    }
};

// REC: the staging prologue behind the record `rec` (conv_pair2_rec.h); else the struct-argument prologue.  Both
// leave the same LDS image, and the MFMA phases and epilogues below are one code: the same bits.
template <int KA, int SA, int KB, int TH, int CINMAX, bool REG, bool REC, bool MS = false>
__device__ __forceinline__ void pair2_body(const esm_conv_desc& a, const esm_conv_desc& bd, const P2Rec& rec) {
    using G = P2Geo<KA, SA, KB, TH>;
    constexpr int NA = G::NA, IR = G::IR, IC = G::IC, ICP = G::ICP, ICS = G::ICS, AR = G::AR, ACS = G::ACS;
    constexpr int TA = KA * KA, TB = KB * KB;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* in = lds;                          // [CINMAX][IR][ICP] (channel stride ICS)
    float* wa = in + CINMAX * ICS;            // [TA][CINMAX][16]
    float* wb = wa + TA * CINMAX * 16;        // [TB][16][16]
    float* at = wb + TB * 256;                // [16][NA][AR] (channel stride ACS)
    float* ep = at + 16 * ACS;                // scaleA, shiftA, scaleB, shiftB [16] each

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 15, kq = lane >> 4;
    constexpr int VB = 16 - KB + 1;
    const Blk3 bk_ = xcd_block(REC ? rec.xcd : (a.hint & kHintXcd) != 0);
    const int b = bk_.z;
    const int yb0 = bk_.y * TH, xb0 = bk_.x * VB;
    const int pb = REC ? rec.pb : bd.ph;
    const int ya0 = yb0 - pb, xa0 = xb0 - pb;                 // convA tile origin
    const int yi0 = ya0 * SA - (REC ? rec.pa : a.ph), xi0 = xa0 * SA - (REC ? rec.pa : a.pw);  // staged input origin
    const int cin = REC ? rec.Cin : a.Cin;
    P2Out eo;
    if constexpr (REC) {
        P2Stage<KA, SA, KB, TH, CINMAX, REG, MS> stg;
        stg.load(rec, tid, bk_, yi0, xi0);
        __builtin_amdgcn_sched_barrier(0);  // every load issued before the first LDS store
        // the output side, loaded from here on: every staging load is issued, and no wait ahead of them covered it
        // (the record's dwords are the leading arguments: `a` sits at byte 4 * kPair2RecDwords, `bd` behind it)
        static_assert(alignof(esm_conv_desc) <= 8 && sizeof(esm_conv_desc) % 8 == 0, "the descriptors behind the record");
        unsigned aoff = 4 * kPair2RecDwords;
        asm volatile("" : "+s"(aoff));
        const unsigned boff = aoff + static_cast<unsigned>(sizeof(esm_conv_desc));
#define ESM_A(T, f) kernarg_at<T>(aoff + offsetof(esm_conv_desc, f))
#define ESM_B(T, f) kernarg_at<T>(boff + offsetof(esm_conv_desc, f))
        // (oc, oh: the low halves, as the struct-argument prologue's static_cast<int> takes them)
        eo = {ESM_B(float*, out), ESM_B(int64_t, ob), ESM_B(int32_t, oc), ESM_B(int32_t, oh), rec.CoutB,
              ESM_B(int32_t, Ho), ESM_B(int32_t, Wo), ESM_A(int32_t, Ho), ESM_A(int32_t, Wo)};
#undef ESM_A
#undef ESM_B
        __builtin_amdgcn_sched_barrier(0);
        stg.store(in, wa, wb, ep, tid);
    } else {
    eo = {bd.out, bd.ob, static_cast<int>(bd.oc), static_cast<int>(bd.oh), bd.Cout, bd.Ho, bd.Wo, a.Ho, a.Wo};
    // ---- stage: input window (zero outside the input and past Cin), weights, BN affines.  The sources'
    //      pointers / strides are read once as wave-uniform values and selected per element in
    //      registers (indexing a.src[] by a per-lane value would re-load them from the kernarg
    //      segment for every element).
    const int ns = a.nsrc;
    const float* sp0 = a.src[0].ptr + b * a.src[0].sb;
    const float* sp1 = ns > 1 ? a.src[1].ptr + b * a.src[1].sb : sp0;
    const float* sp2 = ns > 2 ? a.src[2].ptr + b * a.src[2].sb : sp0;
    const int c0 = a.src[0].C, c01 = c0 + (ns > 1 ? a.src[1].C : 0);
    const int sc0 = static_cast<int>(a.src[0].sc), sh0 = static_cast<int>(a.src[0].sh);
    const int sc1 = ns > 1 ? static_cast<int>(a.src[1].sc) : sc0, sh1 = ns > 1 ? static_cast<int>(a.src[1].sh) : sh0;
    const int sc2 = ns > 2 ? static_cast<int>(a.src[2].sc) : sc0, sh2 = ns > 2 ? static_cast<int>(a.src[2].sh) : sh0;
    constexpr int NIN = CINMAX * IR * IC;
    constexpr int PI = (NIN + kP2Threads - 1) / kP2Threads;
    float vi[PI];
    if constexpr (!REG) {
#pragma unroll
        for (int i = 0; i < PI; ++i) {
            const int e = i * kP2Threads + tid;
            const int q = e % IC, r = (e / IC) % IR, c = e / (IC * IR);
            const int yi = yi0 + r, xi = xi0 + q;
            const bool s1 = c >= c0, s2 = c >= c01;
            const float* base = s2 ? sp2 : (s1 ? sp1 : sp0);
            const int cl = c - (s2 ? c01 : (s1 ? c0 : 0));
            const int scs = s2 ? sc2 : (s1 ? sc1 : sc0), shs = s2 ? sh2 : (s1 ? sh1 : sh0);
            const bool ok = e < NIN && c < cin && yi >= 0 && yi < a.Hi && xi >= 0 && xi < a.Wi;
            const float v = base[ok ? cl * scs + yi * shs + xi : 0];
            vi[i] = ok ? v : 0.f;
        }
    }
    constexpr int NWA = TA * CINMAX * 16;
    constexpr int PWA = (NWA + kP2Threads - 1) / kP2Threads;
    float vwa[PWA];
#pragma unroll
    for (int i = 0; i < PWA; ++i) {
        const int e = i * kP2Threads + tid;
        const int co = e & 15, c = (e >> 4) % CINMAX, tap = e / (16 * CINMAX);
        const bool ok = e < NWA && c < cin && co < a.Cout;
        const float v = a.w[ok ? (static_cast<long long>(tap) * a.cin_pad + c) * a.cout_pad + co : 0];
        vwa[i] = ok ? v : 0.f;
    }
    constexpr int NWB = TB * 256;
    constexpr int PWB = NWB / kP2Threads;
    float vwb[PWB];
#pragma unroll
    for (int i = 0; i < PWB; ++i) {
        const int e = i * kP2Threads + tid;
        const int co = e & 15, c = (e >> 4) & 15, tap = e >> 8;
        const bool ok = c < bd.Cin && co < bd.Cout;
        const float v = bd.w[ok ? (static_cast<long long>(tap) * bd.cin_pad + c) * bd.cout_pad + co : 0];
        vwb[i] = ok ? v : 0.f;
    }
    float vep = 0.f;
    if (tid < 64) {  // scaleA, shiftA, scaleB, shiftB: wave-uniform pointers, selected per lane
        const int k = tid >> 4, c = tid & 15;
        const float* p = k == 0 ? a.scale : (k == 1 ? a.shift : (k == 2 ? bd.scale : bd.shift));
        const int cn = k < 2 ? a.Cout : bd.Cout;
        const bool ok = p != nullptr && c < cn;
        const float v = (ok ? p : a.w)[ok ? c : 0];
        vep = ok ? v : ((k & 1) ? 0.f : 1.f);
    }
    if constexpr (REG) {
        // after the weight loads (the regression's adds and the map's store wait for the cost planes, the
        // weights' loads need not); channel 0 only (Cin 1), the other staged channels zero.  The map is
        // written once per pixel by the tile that owns it: rows [yb0, yb0 + TH) and columns [xb0, xb0 + VB),
        // the edge tiles extended to the map's edges (their windows cover them: launch_p2)
#pragma unroll
        for (int i = 0; i < PI; ++i) {
            const int e = i * kP2Threads + tid;
            const int q = e % IC, r = (e / IC) % IR, c = e / (IC * IR);
            const int yi = yi0 + r, xi = xi0 + q;
            vi[i] = 0.f;
            if (e < NIN && c == 0 && yi >= 0 && yi < a.Hi && xi >= 0 && xi < a.Wi) {
                const float v = regress_px(sp0 + yi * sh0 + xi, a.src[0].C, sc0);
                vi[i] = v;
                const bool own_y = (bk_.y == 0 || yi >= yb0) && (bk_.y == static_cast<int>(gridDim.y) - 1 || yi < yb0 + TH);
                const bool own_x = (bk_.x == 0 || xi >= xb0) && (bk_.x == static_cast<int>(gridDim.x) - 1 || xi < xb0 + VB);
                if (own_y && own_x) a.out[b * a.ob + yi * a.oh + xi] = v;
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);  // every load issued before the first LDS store
#pragma unroll
    for (int i = 0; i < PI; ++i) {
        const int e = i * kP2Threads + tid;
        if (e < NIN) in[(e / (IC * IR)) * ICS + ((e / IC) % IR) * ICP + e % IC] = vi[i];
    }
#pragma unroll
    for (int i = 0; i < PWA; ++i) {
        const int e = i * kP2Threads + tid;
        if (e < NWA) wa[e] = vwa[i];
    }
#pragma unroll
    for (int i = 0; i < PWB; ++i) wb[i * kP2Threads + tid] = vwb[i];
    if (tid < 64) ep[tid] = vep;
    }
    __syncthreads();

    // ---- convA on the tile + halo: row i of the tile = convA output row ya0 + i
    for (int i = wave; i < NA; i += kP2Threads / 64) {
        floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
        const float* ib = in + kq * ICS + i * SA * ICP + n * SA;
        const float* wp = wa + kq * 16 + n;
        const int kca = (cin + 3) >> 2;
        // accumulator indices stay compile-time (a runtime index turns every MFMA into a select chain
        // over the accumulators): two chains alternate by tap, or by channel group for 1x1 convA
        if constexpr (TA > 1) {
            if (cin == 1) {
                // one input channel (the dm<t>.0 heads): the taps fill k, 4 per MFMA (7 MFMAs per row for 5x5,
                // not 25 with 3 zero channels each); lane group kq takes tap 4 kc + kq
                const float* ib0 = in + i * SA * ICP + n * SA;
#pragma unroll
                for (int kc = 0; kc < (TA + 3) / 4; ++kc) {
                    const int t = 4 * kc + kq;
                    const bool tv = t < TA;
                    const int tt = tv ? t : 0;
                    const float bv = ib0[(tt / KA) * ICP + tt % KA];
                    const float av = wa[tt * CINMAX * 16 + n];
                    acc[kc & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(tv ? av : 0.f, tv ? bv : 0.f, acc[kc & 1], 0, 0, 0);
                }
            } else {
                for (int kc = 0; kc < kca; ++kc) {
#pragma unroll
                    for (int t = 0; t < TA; ++t) {
                        const int ky = t / KA, kx = t % KA;
                        const float bv = ib[4 * kc * ICS + ky * ICP + kx];
                        const float av = wp[(t * CINMAX + 4 * kc) * 16];
                        acc[t & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[t & 1], 0, 0, 0);
                    }
                }
            }
        } else {
            for (int kc = 0; kc < kca; kc += 2) {
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[4 * kc * 16], ib[4 * kc * ICS], acc[0], 0, 0, 0);
                if (kc + 1 < kca)
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wp[4 * (kc + 1) * 16], ib[4 * (kc + 1) * ICS], acc[1],
                                                                  0, 0, 0);
            }
        }
        const int ya = ya0 + i, xa = xa0 + n;
        const bool inside = ya >= 0 && ya < eo.aHo && xa >= 0 && xa < eo.aWo;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = 4 * kq + j;
            const float v = act_t<ESM_ACT_GELU>((acc[0][j] + acc[1][j]) * ep[co] + ep[16 + co], 0);
            at[co * ACS + i * AR + n] = inside ? v : 0.f;
        }
    }
    __syncthreads();

    // ---- convB from LDS: output row yb0 + t, columns xb0 .. xb0 + VB - 1
    for (int t = wave; t < TH; t += kP2Threads / 64) {
        floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
        const float* ab = at + kq * ACS + t * AR + n;
        const float* wp = wb + kq * 16 + n;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc)
#pragma unroll
            for (int tp = 0; tp < TB; ++tp) {
                const int dy = tp / KB, dx = tp % KB;
                const float bv = ab[4 * kc * ACS + dy * AR + dx];
                const float av = wp[(tp * 16 + 4 * kc) * 16];
                acc[tp & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[tp & 1], 0, 0, 0);
            }
        const int yb = yb0 + t, xb = xb0 + n;
        const bool ok = yb < eo.Ho && xb < eo.Wo && n < VB;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
            eo.out + b * eo.ob, static_cast<short>(0), 4 * ((eo.Cout - 1) * eo.oc + (eo.Ho - 1) * eo.oh + eo.Wo), 0x00020000);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int co = 4 * kq + j;
            const float v = act_t<ESM_ACT_GELU>((acc[0][j] + acc[1][j]) * ep[32 + co] + ep[48 + co], 0);
            const unsigned o = (ok && co < eo.Cout) ? 4u * (co * eo.oc + yb * eo.oh + xb) : kOOB;
            store_b32(__float_as_uint(v), ro, static_cast<int>(o), 0);
        }
    }
}

template <int KA, int SA, int KB, int TH, int CINMAX, bool REG>
__global__ void __launch_bounds__(kP2Threads) pair2_kernel(const esm_conv_desc a, const esm_conv_desc bd) {
    pair2_body<KA, SA, KB, TH, CINMAX, REG, false>(a, bd, P2Rec{});
}

// The same kernel behind the staging record: 20 leading scalar dwords (conv_pair2_rec.h), then the descriptors
template <int KA, int SA, int KB, int TH, int CINMAX, bool REG, bool MS>
__global__ void __launch_bounds__(kP2Threads) pair2_rec_kernel(ESM_REC_PARAMS(20), const esm_conv_desc a,
                                                              const esm_conv_desc bd) {
    const P2Rec r = pair2_record_unpack(ESM_REC_DWORDS(20));
    pair2_body<KA, SA, KB, TH, CINMAX, REG, true, MS>(a, bd, r);
}

// Whether an LDS-form launch goes behind the staging record, and the record: every pair it can describe unless
// PAIR_NO_RECORD in convB's hint asks for the struct-argument kernel (A/B, tests)
inline bool pair2_use_record(const esm_conv_desc& a, const esm_conv_desc& b, unsigned (&rec)[kPair2RecDwords]) {
    return !(b.hint & ESM_HINT_PAIR_NO_RECORD) && pair2_record_pack(a, b, rec);
}

// Tile rows of an LDS-form launch.  b.hint ROWS(1 / 2 / 3): 2 / 4 / 8 rows (8: <= 16 input channels); 0 automatic:
// 2-row tiles on small maps (more workgroups), 4-row tiles where that still gives >= 256
inline int p2_rows(const esm_conv_desc& a, const esm_conv_desc& b) {
    const long long tiles4 = static_cast<long long>(ceil_div(b.Wo, 16 - b.kh + 1)) * ceil_div(b.Ho, 4) * a.B;
    const int thsel = hint_rows(b);
    if (thsel == 3 && a.Cin <= 16) return 8;
    return (thsel ? thsel == 1 : tiles4 < 256) ? 2 : 4;
}

// What an LDS-form launch with th-row tiles cannot run: a grid past the limits and, with PAIR_REGRESS, a regressed
// map that the windows of the tiles storing it do not cover (P2Geo's IR x IC window: launch_p2 asserts the formulas)
int p2_tile_check(const esm_conv_desc& a, const esm_conv_desc& b, int th) {
    const int vb = 16 - b.kh + 1;
    const int gx = ceil_div(b.Wo, vb), gy = ceil_div(b.Ho, th);
    if (gy < 1 || gy > 65535 || a.B < 1 || a.B > 65535) return arg_error("conv pair: grid too large");
    if (a.hint & ESM_HINT_PAIR_REGRESS) {
        const int ir = (th + b.kh - 2) * a.stride + a.kh, ic = 15 * a.stride + a.kh;
        const int pr = b.ph + a.ph, pc = b.pw + a.pw;
        if (pr < 0 || pc < 0 || th > ir - pr || vb > ic - pc || (gy - 1) * th - pr + ir < a.Hi || (gx - 1) * vb - pc + ic < a.Wi)
            return arg_error("conv pair: regressed map not covered by the tiles");
    }
    return ESM_OK;
}

// a, b: a pair pair2_form named ESM_PAIR_FORM_LDS at TH rows (p2_rows; p2_tile_check passed)
template <int KA, int SA, int KB, int TH, int CINMAX, bool REG = false>
int launch_p2(const esm_conv_desc& a, const esm_conv_desc& b, hipStream_t s) {
    using G = P2Geo<KA, SA, KB, TH>;
    static_assert(G::IR == (TH + KB - 2) * SA + KA && G::IC == 15 * SA + KA, "p2_tile_check's window");
    const size_t lds = sizeof(float) * (static_cast<size_t>(CINMAX) * G::ICS + KA * KA * CINMAX * 16 + KB * KB * 256 +
                                        16 * G::ACS + 64);
    constexpr int VB = 16 - KB + 1;
    const dim3 grid(ceil_div(b.Wo, VB), ceil_div(b.Ho, TH), a.B);
    // behind the record: MS, the window's groups select their source (a second scalar batch); one source needs none
    unsigned rec[kPair2RecDwords];
    constexpr bool MSOK = !REG && CINMAX >= 8;
    if (pair2_use_record(a, b, rec) && (MSOK || a.nsrc == 1)) {
        if constexpr (MSOK) {
            if (a.nsrc > 1) {
                hipLaunchKernelGGL((pair2_rec_kernel<KA, SA, KB, TH, CINMAX, REG, true>), grid, dim3(kP2Threads), lds, s,
                                   ESM_REC_ARGS(20, rec), a, b);
                return check_launch("conv pair");
            }
        }
        hipLaunchKernelGGL((pair2_rec_kernel<KA, SA, KB, TH, CINMAX, REG, false>), grid, dim3(kP2Threads), lds, s,
                           ESM_REC_ARGS(20, rec), a, b);
    } else
        hipLaunchKernelGGL((pair2_kernel<KA, SA, KB, TH, CINMAX, REG>), grid, dim3(kP2Threads), lds, s, a, b);
    return check_launch("conv pair");
}

template <int KA, int SA, int KB>
int launch_p2_k(const esm_conv_desc& a, const esm_conv_desc& b, hipStream_t s) {
    const int th = p2_rows(a, b);
    const bool small = th == 2, tall = th == 8;
    if constexpr (KA == 5 && KB == 3) {
        if (a.hint & ESM_HINT_PAIR_REGRESS) {
            if (tall) return launch_p2<KA, SA, KB, 8, 4, true>(a, b, s);
            return small ? launch_p2<KA, SA, KB, 2, 4, true>(a, b, s) : launch_p2<KA, SA, KB, 4, 4, true>(a, b, s);
        }
    }
    if (tall) return a.Cin <= 4 ? launch_p2<KA, SA, KB, 8, 4>(a, b, s) : launch_p2<KA, SA, KB, 8, 16>(a, b, s);
    if (a.Cin <= 4) return small ? launch_p2<KA, SA, KB, 2, 4>(a, b, s) : launch_p2<KA, SA, KB, 4, 4>(a, b, s);
    if (a.Cin <= 16) return small ? launch_p2<KA, SA, KB, 2, 16>(a, b, s) : launch_p2<KA, SA, KB, 4, 16>(a, b, s);
    if (a.Cin <= 32) return small ? launch_p2<KA, SA, KB, 2, 32>(a, b, s) : launch_p2<KA, SA, KB, 4, 32>(a, b, s);
    if constexpr (KA == 1) {
        if (a.Cin > 48) return small ? launch_p2<KA, SA, KB, 2, 64>(a, b, s) : launch_p2<KA, SA, KB, 4, 64>(a, b, s);
    }
    return small ? launch_p2<KA, SA, KB, 2, 48>(a, b, s) : launch_p2<KA, SA, KB, 4, 48>(a, b, s);
}

}  // namespace

// convA: 2-D, not transposed, k 1/3/5 (stride 1) or 3 (stride 2), <= 48 input channels (64 for k 1; 1..3 sources),
// 16 outputs, BN + GELU, plain output (only convB's output is stored); convB: 2-D k1/k3 stride 1 over
// convA's 16 channels, <= 16 outputs, BN + GELU, plain epilogue.  With PAIR_REGRESS on convA (5x5, one
// input channel, convB 3x3): src[0] is a [B, D, H, W] cost volume (C = D) and convA's input map is its
// disparity_regression (models/submodule.py:211-216), computed per staged pixel and stored once to
// a.out ([B, 1, H, W], strides ob / oh) -- the regression launch of the hot path folded into the
// upsampler's first pair.
bool pair2_lds_ok(const esm_conv_desc& a, const esm_conv_desc& b) {
    const bool a3 = is3d(a), b3 = is3d(b);
    if (a.nsrc < 1 || a.nsrc > ESM_MAX_SRC) return false;
    if (a3 || b3 || a.transposed || b.transposed || a.shuffle > 1 || b.shuffle > 1) return false;
    if (a.Cout != 16 || a.Cin < 1 || a.Cin > (a.kh == 1 ? 64 : 48) || b.Cin != 16 || b.Cout < 1 || b.Cout > 16)
        return false;
    if (!((a.kh == 3 && (a.stride == 1 || a.stride == 2)) || ((a.kh == 1 || a.kh == 5) && a.stride == 1))) return false;
    if (a.ph != a.pw || b.ph != b.pw || b.stride != 1 || (b.kh != 1 && b.kh != 3)) return false;
    if (a.act != ESM_ACT_GELU || b.act != ESM_ACT_GELU) return false;
    if (a.mul || a.res || a.up || a.out2 || a.post_scale != 1.f) return false;
    if (b.mul || b.res || b.up || b.out2 || b.post_scale != 1.f || !b.out) return false;
    if (b.Hi != a.Ho || b.Wi != a.Wo || b.B != a.B) return false;
    if (b.Ho != b.Hi + 2 * b.ph - b.kh + 1 || b.Wo != b.Wi + 2 * b.pw - b.kw + 1) return false;
    if (a.nsrc > 1)
        for (int i = 0; i < a.nsrc; ++i)
            if (a.src[i].C % 4) return false;
    // the struct-argument kernel indexes a source's batch item with an int element offset (the record kernel's
    // narrower limits: pair2_record_pack, which falls back to it)
    for (int i = 0; i < a.nsrc && i < ESM_MAX_SRC; ++i) {
        const esm_src& r = a.src[i];
        if (r.sc < 0 || r.sh < 0 || r.sc >= (1LL << 31) || r.sh >= (1LL << 31)) return false;
        const long long ch = (a.hint & ESM_HINT_PAIR_REGRESS) ? 1 : r.C;  // (the cost volume's planes: below)
        if ((ch - 1) * r.sc + (a.Hi - 1) * r.sh + a.Wi >= (1LL << 31)) return false;
    }
    if (a.hint & ESM_HINT_PAIR_REGRESS) {  // convA 5x5 1 -> 16 over the regressed map, convB 3x3 (dm<t>.0 + .1)
        if (a.kh != 5 || b.kh != 3 || a.Cin != 1 || a.nsrc != 1 || a.src[0].C < 1 || !a.out || a.out == b.out)
            return false;
        if (static_cast<long long>(a.src[0].C) * a.src[0].sc >= (1LL << 31) || a.src[0].sh >= (1 << 28)) return false;
    }
    const long long last = (b.Cout - 1) * b.oc + (b.Ho - 1) * b.oh + b.Wo;
    return 4 * last < static_cast<long long>(kOOB) && b.oc < (1 << 28) && b.oh < (1 << 28);
}

bool pairk_ok(const esm_conv_desc& a, const esm_conv_desc& b);                    // conv_pairk.hip
int pairk_tile_check(const esm_conv_desc& a, const esm_conv_desc& b);             // conv_pairk.hip
int launch_pairk(const esm_conv_desc& a, const esm_conv_desc& b, hipStream_t s);  // conv_pairk.hip

// The form esm_conv_pair2_f32 takes for the pair: ESM_PAIR_FORM_LDS or ESM_PAIR_FORM_KSPLIT, or ESM_ERR_ARG with the
// message set.  The K-split form (conv_pairk.hip: 3x3(x3) pairs, 2-D and 3-D, up to 32 couts) where PAIRK in b.hint
// asks for it, and automatically for what only it runs; never with the regression source.  launch_pair2 switches
// over the result, esm_conv_pair2_form reports it and esm_pair2_record_pack answers for the LDS form only.
int pair2_form(const esm_conv_desc& a, const esm_conv_desc& b) {
    const bool lds = pair2_lds_ok(a, b);
    int rc;
    if (((b.hint & ESM_HINT_PAIRK) || !lds) && !(a.hint & ESM_HINT_PAIR_REGRESS) && pairk_ok(a, b))
        return (rc = pairk_tile_check(a, b)) != ESM_OK ? rc : ESM_PAIR_FORM_KSPLIT;
    if (!lds) return arg_error("conv pair: unsupported pair");
    return (rc = p2_tile_check(a, b, p2_rows(a, b))) != ESM_OK ? rc : ESM_PAIR_FORM_LDS;
}

int launch_pair2(const esm_conv_desc& a, const esm_conv_desc& b, hipStream_t s) {
    const int form = pair2_form(a, b);
    if (form < 0) return form;
    if (form == ESM_PAIR_FORM_KSPLIT) return launch_pairk(a, b, s);
    if (a.kh == 5) return b.kh == 3 ? launch_p2_k<5, 1, 3>(a, b, s) : launch_p2_k<5, 1, 1>(a, b, s);
    if (a.kh == 1) return b.kh == 3 ? launch_p2_k<1, 1, 3>(a, b, s) : launch_p2_k<1, 1, 1>(a, b, s);
    if (a.stride == 2) return b.kh == 3 ? launch_p2_k<3, 2, 3>(a, b, s) : launch_p2_k<3, 2, 1>(a, b, s);
    return b.kh == 3 ? launch_p2_k<3, 1, 3>(a, b, s) : launch_p2_k<3, 1, 1>(a, b, s);
}

}  // namespace conv
}  // namespace esm

extern "C" int esm_pair2_record_pack(const esm_conv_desc* a, const esm_conv_desc* b, uint32_t rec[20], int64_t fields[24]) {
    namespace C = esm::conv;
    static_assert(C::kPair2RecDwords == 20 && C::kPair2RecFields == 24, "the header's array sizes");
    if (!a || !b || !rec || !fields) return esm::arg_error("pair2_record_pack: null argument");
    // the launch launch_pair2 makes: the LDS form (not the K-split one), behind the record or not
    if (C::pair2_form(*a, *b) != ESM_PAIR_FORM_LDS) return 0;
    unsigned d[C::kPair2RecDwords];
    if (!C::pair2_use_record(*a, *b, d)) return 0;
    const C::P2Rec r = C::pair2_record_unpack(d);
    const int64_t f[C::kPair2RecFields] = {C::ptr_field(r.src0), C::ptr_field(r.wa), C::ptr_field(r.wb), r.sb0, r.sc, r.sh,
                                           r.Wi, r.Hi, r.Cin, r.pa, r.pb, r.CoutB, r.nsrc, r.xcd, r.D, C::ptr_field(r.src1),
                                           C::ptr_field(r.src2), r.sb1, r.sb2, r.C0, r.C01, C::ptr_field(r.out), r.ob, r.oh};
    return C::record_export(d, f, rec, fields);
}

extern "C" int esm_conv_pair2_form(const esm_conv_desc* a, const esm_conv_desc* b) {
    if (!a || !b) return esm::arg_error("conv pair: null descriptor");
    return esm::conv::pair2_form(*a, *b);
}

extern "C" int esm_conv_pair2_f32(const esm_conv_desc* a, const esm_conv_desc* b, void* stream) {
    if (!a || !b) return esm::arg_error("conv pair: null descriptor");
    return esm::conv::launch_pair2(*a, *b, esm::as_stream(stream));
}
