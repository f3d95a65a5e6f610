// Two consecutive BasicConvs (3x3 or 3x3x3) in one launch, K-split form: the pair kernel of conv_pair2.hip
// with the latency structure of the lean form (conv_small.hip) in both phases.
//   y = GELU(BN_B(convB(GELU(BN_A(convA(cat(sources)))))))
// convA: k3 stride 1 / 2 pad 1, 2-D or 3-D, <= 48 input channels over up to 3 sources, <= 32 outputs;
// convB: k3 stride 1 pad 1 over convA's outputs, <= 32 outputs.  The pairs of the hourglasses' levels
// (models/ESMStereo.py:129-182 aggregation conv1 / conv2 / conv3, :185-239 up_refinement conv2 / conv3)
// and spx_<t>.0 -> .1 (:247-259).  On the small 2-D maps each launch of such a pair sits at the lean form's
// latency floor and the pair measured faster than the two (engine.pairk_auto: S-K ref2x.conv2 / conv3 and
// spx_2x, 5.9-8.6 us against 9.1-9.6); the 3-D pairs and the maps from 48x156 up measured slower and stay
// two launches.
//
// A workgroup owns one 16-column tile of convA (14 valid convB columns), TH convB output rows of one
// output plane and batch item.
//   Phase A: convA on the (TH + 2) rows x (3 planes in 3-D) of 16-column row segments convB's window
//     needs.  The unit of work is a wave-task = one row segment x one 4-channel group of the K reduction:
//     every B operand (one buffer_load per tap, borders by kOOB marks: conv_direct.h) and every weight of
//     the task is requested before its first MFMA; TAPS x MT MFMAs on two alternating accumulators.
//     Segments wholly outside convA's extent are not computed.  Tasks go round-robin over the NW waves.
//     The partial tiles meet in LDS ([task][cout][16 columns]) and are summed in group order (fixed:
//     deterministic); BN + GELU; positions outside convA's extent are zeros (convB's padding).  The result
//     is an LDS tile [cout][plane][row][18].
//   Phase B: wave-task = one output row x one 4-channel group (x one plane tap in 3-D): 9 ds_reads and
//     9 x MT weight loads, then 9 x MT MFMAs.  The first task's weights are requested before the barrier
//     that ends phase A's MFMAs, so their round trip hides behind phase A's reduction.  Fixed-order sum in
//     LDS, BN + GELU, buffer stores (kOOB for couts past Cout, columns past the tile or the map).
#include <algorithm>

#include "conv_direct.h"
#include "kernarg_rec.h"

namespace esm {
namespace conv {
namespace {

constexpr int kPkAR = 18;  // LDS row pitch of convA's tile (16 columns + convB's dx overrun), as pair2_kernel
constexpr int kPkVB = 14;  // valid convB columns per tile
constexpr size_t kPkMaxLds = 64 * 1024;
// waves per workgroup.  16 measured faster than 8 on every pair of the S-K chain (in the replayed graph, us:
// 6.1 vs 7.0 and 6.0 vs 6.9 on the 24x78 / 12x39 stride-2 pairs, 8.7 vs 9.7 on spx_2x, 11.0 vs 12.6 / 13.1 vs
// 14.8 / 16.9 vs 19.3 on the 3-D pairs), so the 8-wave variant is gone
constexpr int kPkWaves = 16;

inline int pk_acs(int np, int na) {  // channel stride of the tile: = 16 (mod 32), conflict-free k-quarter reads
    const int s = np * na * kPkAR;
    return s + ((16 - s % 32) + 32) % 32;
}

struct PkGeo {
    int th;                        // convB output rows per workgroup
    int acs;                       // channel stride of convA's LDS tile (floats)
    int red;                       // floats of the partial-tile region
    unsigned m_ga, m_gb, m_do;     // reciprocals of the channel group counts and of Do
    unsigned m_ca, m_cb;           // reciprocals of 16 x the (4-aligned) cout counts
};

// convB's first wave-task's weights: 9 taps (of plane tap dz in 3-D) x MT cout tiles of channel group g
template <int MT>
__device__ __forceinline__ void pk_load_wb(float (&av)[9][MT], __amdgpu_buffer_rsrc_t wrs, unsigned wl, int wtap,
                                           int cout_pad, int g, int dz) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            av[t][mt] = buf_load_s(wrs, wl, 4 * ((dz * 9 + t) * wtap + 4 * g * cout_pad + 16 * mt));
}

template <bool D3, int SA, int MT, int NW>
__global__ void __launch_bounds__(64 * NW) pairk_kernel(const esm_conv_desc a, const esm_conv_desc bd, const PkGeo geo) {
    constexpr int NP = D3 ? 3 : 1;   // convA planes under convB's window
    constexpr int KDT = D3 ? 3 : 1;
    constexpr int TAPS = KDT * 9;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* red = lds;                 // [task][cout][16]
    float* at = red + geo.red;        // [cout][plane][row][kPkAR]
    const int TH = geo.th, NA = TH + 2, ACS = geo.acs;
    const int GA = (a.Cin + 3) >> 2, GB = (bd.Cin + 3) >> 2;
    const int CPA = 4 * ((a.Cout + 3) >> 2), CPB = 4 * ((bd.Cout + 3) >> 2);
    float* ep = at + CPA * ACS;       // scaleA, shiftA, scaleB, shiftB [32] each

    const int tid = static_cast<int>(threadIdx.x);
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, kq = lane >> 4;
    const Blk3 bk_ = xcd_block((a.hint & kHintXcd) != 0);
    const int xb0 = bk_.x * kPkVB, yb0 = bk_.y * TH;
    const int b = magic_div(bk_.z, geo.m_do);
    const int zb = bk_.z - b * bd.Do;

    // BN affines of both convs -> LDS (read behind phase A's barrier)
    if (tid < 128) {
        const int k = tid >> 5, c = tid & 31;
        const float* p = k == 0 ? a.scale : (k == 1 ? a.shift : (k == 2 ? bd.scale : bd.shift));
        const int cn = k < 2 ? a.Cout : bd.Cout;
        const bool ok = p != nullptr && c < cn;
        const float v = (ok ? p : a.w)[ok ? c : 0];
        ep[tid] = ok ? v : ((k & 1) ? 0.f : 1.f);
    }

    // ---- phase A: the valid planes [plo, phi) and rows [ilo, ihi) of the tile (convA plane zb - 1 + p, row
    //      yb0 - 1 + i), compacted into wave-tasks (segment, channel group)
    const int plo = D3 ? max(0, 1 - zb) : 0, phi = D3 ? min(3, a.Do + 1 - zb) : 1;
    const int ilo = max(0, 1 - yb0), ihi = min(NA, a.Ho + 1 - yb0);
    const int nvr = ihi - ilo;
    const int ntask = (phi - plo) * nvr * GA;

    const int xa = xb0 - 1 + n16;  // convA column of this lane
    unsigned xoff[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int xi = xa * SA - a.pw + t;
        xoff[t] = (xa >= 0 && xa < a.Wo && xi >= 0 && xi < a.Wi) ? 4u * xi : kOOB;
    }
    const int wtap = a.cin_pad * a.cout_pad;
    const __amdgpu_buffer_rsrc_t wrs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), static_cast<short>(0), 4 * TAPS * wtap, 0x00020000);
    const unsigned wl = 4u * (kq * a.cout_pad + n16);
    const int ns = a.nsrc;
    const int lo1 = a.src[0].C, lo2 = lo1 + (ns > 1 ? a.src[1].C : 0);

    // One task's loads in flight at a time.  Requesting three 2-D tasks' operands at once (9 (1 + MT) registers
    // each) measured slower, 8.2-8.6 vs 5.9-6.4 us on the 12-task pairs whose spare slots repeated loads: the phase
    // is paced by the vector-memory instructions a CU issues, not by their round trips.
    for (int t = wave; t < ntask; t += NW) {
        const int seg = magic_div(t, geo.m_ga);
        const int g = t - seg * GA;
        const int pp = (seg >= nvr ? 1 : 0) + (seg >= 2 * nvr ? 1 : 0);
        const int za = zb - 1 + plo + pp, ya = yb0 - 1 + ilo + (seg - pp * nvr);
        const int c0 = 4 * g;
        // the group's source (4-channel aligned splits): named-field selects, no runtime index
        const int s = (ns > 1 && c0 >= lo1) ? ((ns > 2 && c0 >= lo2) ? 2 : 1) : 0;
        const int lo = s == 0 ? 0 : (s == 1 ? lo1 : lo2);
        const float* sp = s == 0 ? a.src[0].ptr : (s == 1 ? a.src[1].ptr : a.src[2].ptr);
        const int sC = s == 0 ? a.src[0].C : (s == 1 ? a.src[1].C : a.src[2].C);
        const long long sb = s == 0 ? a.src[0].sb : (s == 1 ? a.src[1].sb : a.src[2].sb);
        const int sc = static_cast<int>(s == 0 ? a.src[0].sc : (s == 1 ? a.src[1].sc : a.src[2].sc));
        const int sd = static_cast<int>(s == 0 ? a.src[0].sd : (s == 1 ? a.src[1].sd : a.src[2].sd));
        const int sh = static_cast<int>(s == 0 ? a.src[0].sh : (s == 1 ? a.src[1].sh : a.src[2].sh));
        const int span = 4 * ((sC - 1) * sc + (D3 ? (a.Di - 1) * sd : 0) + (a.Hi - 1) * sh + a.Wi);
        const __amdgpu_buffer_rsrc_t rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(sp + b * sb), static_cast<short>(0), span, 0x00020000);
        const int cl = c0 - lo + kq;
        const unsigned chv = (c0 + kq < a.Cin && cl < sC) ? 4u * cl * sc : kOOB;

        float bv[TAPS], av[TAPS][MT];
#pragma unroll
        for (int dz = 0; dz < KDT; ++dz) {
            const int zi = D3 ? za * SA - a.pd + dz : 0;
            const bool zok = !D3 || (zi >= 0 && zi < a.Di);
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int yi = ya * SA - a.ph + dy;
                const int roff = (zok && yi >= 0 && yi < a.Hi) ? 4 * ((D3 ? zi * sd : 0) + yi * sh) : static_cast<int>(kOOB);
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int tap = (dz * 3 + dy) * 3 + dx;
                    bv[tap] = buf_load_s(rs, chv + xoff[dx], roff);
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        av[tap][mt] = buf_load_s(wrs, wl, 4 * (tap * wtap + c0 * a.cout_pad + 16 * mt));
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // every load of the task in flight before the first MFMA
        floatx4 acc[2][MT];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[c][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[tap & 1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[tap][mt], bv[tap], acc[tap & 1][mt], 0, 0, 0);
        float* rp = red + t * CPA * 16 + n16;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = 16 * mt + 4 * kq + j;
                if (co < CPA) rp[co * 16] = acc[0][mt][j] + acc[1][mt][j];
            }
    }

    // convB's weights of this wave's first task: requested before the barrier
    const int NPB = D3 ? 3 : 1;
    const int ntb = TH * GB * NPB;
    const int wtapb = bd.cin_pad * bd.cout_pad;
    const __amdgpu_buffer_rsrc_t wrsb =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bd.w), static_cast<short>(0), 4 * TAPS * wtapb, 0x00020000);
    const unsigned wlb = 4u * (kq * bd.cout_pad + n16);
    float avb[9][MT];
    {
        const int tg = magic_div(wave, D3 ? 0x55555556u : 0u);  // wave / NPB
        const int dz = wave - tg * NPB;
        const int g = tg - magic_div(tg, geo.m_gb) * GB;
        if (wave < ntb) pk_load_wb<MT>(avb, wrsb, wlb, wtapb, bd.cout_pad, g, dz);
    }
    __syncthreads();

    // ---- convA's epilogue: element (segment, cout, column) = fixed-order sum of its GA partial tiles, BN + GELU;
    //      zero outside convA's extent (convB's zero padding) and in the segments not computed
    {
        const int nel = NP * NA * CPA * 16;
        for (int e = tid; e < nel; e += 64 * NW) {
            const int sgi = magic_div(e, geo.m_ca);
            const int r = e - sgi * CPA * 16;
            const int co = r >> 4, n = r & 15;
            const int p = D3 ? (sgi >= NA ? 1 : 0) + (sgi >= 2 * NA ? 1 : 0) : 0;
            const int i = sgi - p * NA;
            const int xc = xb0 - 1 + n;
            const bool ok = p >= plo && p < phi && i >= ilo && i < ihi && xc >= 0 && xc < a.Wo && co < a.Cout;
            float v = 0.f;
            if (ok) {
                const float* rp = red + ((p - plo) * nvr + (i - ilo)) * GA * CPA * 16 + r;
                v = rp[0];
                for (int g = 1; g < GA; ++g) v = v + rp[g * CPA * 16];
                v = gelu_erf(v * ep[co] + ep[32 + co]);
            }
            at[co * ACS + sgi * kPkAR + n] = v;
        }
    }
    __syncthreads();

    // ---- phase B: wave-task (output row t, channel group g, plane tap dz)
    for (int tb = wave; tb < ntb; tb += NW) {
        const int tg = magic_div(tb, D3 ? 0x55555556u : 0u);
        const int dz = tb - tg * NPB;
        const int tr = magic_div(tg, geo.m_gb);
        const int g = tg - tr * GB;
        if (tb != wave) pk_load_wb<MT>(avb, wrsb, wlb, wtapb, bd.cout_pad, g, dz);
        const float* ab = at + (4 * g + kq) * ACS + (dz * NA + tr) * kPkAR + n16;
        float bvb[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) bvb[t] = ab[(t / 3) * kPkAR + t % 3];
        __builtin_amdgcn_sched_barrier(0);
        floatx4 acc[2][MT];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) acc[c][mt] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
                acc[t & 1][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(avb[t][mt], bvb[t], acc[t & 1][mt], 0, 0, 0);
        float* rp = red + tb * CPB * 16 + n16;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int co = 16 * mt + 4 * kq + j;
                if (co < CPB) rp[co * 16] = acc[0][mt][j] + acc[1][mt][j];
            }
    }
    __syncthreads();

    // ---- convB's epilogue: element (row, cout, column) = fixed-order sum over (group, plane tap), BN + GELU, store
    {
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
            bd.out + b * bd.ob, static_cast<short>(0),
            4 * ((bd.Cout - 1) * static_cast<int>(bd.oc) + (D3 ? (bd.Do - 1) * static_cast<int>(bd.od) : 0) +
                 (bd.Ho - 1) * static_cast<int>(bd.oh) + bd.Wo),
            0x00020000);
        const int nel = TH * CPB * 16;
        const int per = GB * NPB;
        for (int e = tid; e < nel; e += 64 * NW) {
            const int tr = magic_div(e, geo.m_cb);
            const int r = e - tr * CPB * 16;
            const int co = r >> 4, n = r & 15;
            const float* rp = red + tr * per * CPB * 16 + r;
            float v = rp[0];
            for (int k = 1; k < per; ++k) v = v + rp[k * CPB * 16];
            v = gelu_erf(v * ep[64 + co] + ep[96 + co]);
            const int yb = yb0 + tr, xb = xb0 + n;
            const bool ok = n < kPkVB && xb < bd.Wo && yb < bd.Ho && co < bd.Cout;
            const unsigned vo = ok ? 4u * (co * static_cast<int>(bd.oc) + xb) : kOOB;
            const int so = 4 * ((D3 ? zb * static_cast<int>(bd.od) : 0) + min(yb, bd.Ho - 1) * static_cast<int>(bd.oh));
            store_b32(__float_as_uint(v), ro, static_cast<int>(vo), so);
        }
    }
}

// LDS bytes of a tile of th rows; the geometry the kernel takes
size_t pk_geo(const esm_conv_desc& a, const esm_conv_desc& b, bool d3, int th, PkGeo* geo) {
    const int np = d3 ? 3 : 1, na = th + 2;
    const int ga = (a.Cin + 3) / 4, gb = (b.Cin + 3) / 4;
    const int cpa = 4 * ((a.Cout + 3) / 4), cpb = 4 * ((b.Cout + 3) / 4);
    const int segs = std::min(np, a.Do) * std::min(na, a.Ho);
    const int red = std::max(segs * ga * cpa * 16, th * gb * np * cpb * 16);
    const int acs = pk_acs(np, na);
    if (geo) *geo = PkGeo{th, acs, red, magic_u32(ga), magic_u32(gb), magic_u32(b.Do), magic_u32(cpa * 16), magic_u32(cpb * 16)};
    return sizeof(float) * (static_cast<size_t>(red) + static_cast<size_t>(cpa) * acs + 128);
}

// Tile rows (b.hint ROWS(1 / 2 / 3): 1 / 2 / 4; 0 automatic): the fewest rows that keep the grid within one
// workgroup per CU (phase A's chain is (TH + 2) x planes x groups wave-tasks long), then what LDS holds (one row
// always fits: pairk_ok)
int pk_rows(const esm_conv_desc& a, const esm_conv_desc& b) {
    const int tiles_w = ceil_div(b.Wo, kPkVB);
    const long long planes = static_cast<long long>(b.Do) * a.B;
    const int sel = hint_rows(b);
    int th = sel == 3 ? 4 : sel;
    if (!th) {
        th = 1;
        while (th < 4 && tiles_w * static_cast<long long>(ceil_div(b.Ho, th)) * planes > 256) th *= 2;
    }
    while (th > 1 && pk_geo(a, b, is3d(a), th, nullptr) > kPkMaxLds) th /= 2;
    return th;
}

// a, b: a pair pair2_form named ESM_PAIR_FORM_KSPLIT (pairk_ok and pairk_tile_check passed)
template <bool D3, int SA, int MT>
int launch_pk(const esm_conv_desc& a, const esm_conv_desc& b, hipStream_t s) {
    const int th = pk_rows(a, b);
    PkGeo geo;
    const size_t lds = pk_geo(a, b, D3, th, &geo);
    const dim3 grid(ceil_div(b.Wo, kPkVB), ceil_div(b.Ho, th), static_cast<unsigned>(b.Do) * a.B);
    hipLaunchKernelGGL((pairk_kernel<D3, SA, MT, kPkWaves>), grid, dim3(64 * kPkWaves), lds, s, a, b, geo);
    return check_launch("conv pair (K-split)");
}

}  // namespace

// The pairs the K-split form runs: convA k3 (x3) stride 1 / 2 pad 1, <= 48 input channels over 1..3 sources
// (4-channel multiples when several), <= 32 outputs; convB k3 (x3) stride 1 pad 1 over them, <= 32 outputs;
// BN + GELU and a plain store on both; the one-row tile within LDS.
bool pairk_ok(const esm_conv_desc& a, const esm_conv_desc& b) {
    const bool a3 = is3d(a), b3 = is3d(b);
    if (a3 != b3 || a.transposed || b.transposed || a.shuffle > 1 || b.shuffle > 1) return false;
    if (a.kh != 3 || a.kw != 3 || b.kh != 3 || b.kw != 3 || a.kd != (a3 ? 3 : 1) || b.kd != (a3 ? 3 : 1)) return false;
    if ((a.stride != 1 && a.stride != 2) || b.stride != 1) return false;
    if (a.ph != 1 || a.pw != 1 || b.ph != 1 || b.pw != 1 || (a3 && (a.pd != 1 || b.pd != 1))) return false;
    if (a.Cin < 1 || a.Cin > 48 || a.Cout < 1 || a.Cout > 32 || b.Cin != a.Cout || b.Cout < 1 || b.Cout > 32) return false;
    if (a.act != ESM_ACT_GELU || b.act != ESM_ACT_GELU) return false;
    if (a.mul || a.res || a.up || a.out2 || a.post_scale != 1.f) return false;
    if (b.mul || b.res || b.up || b.out2 || b.post_scale != 1.f || !b.out) return false;
    if (a.nsrc < 1 || a.nsrc > ESM_MAX_SRC || !direct_ok(a)) return false;
    int cs = 0;
    for (int i = 0; i < a.nsrc; ++i) cs += a.src[i].C;
    if (cs < a.Cin) return false;
    if (b.B != a.B || b.Di != a.Do || b.Hi != a.Ho || b.Wi != a.Wo || b.Do != b.Di || b.Ho != b.Hi || b.Wo != b.Wi) return false;
    if (a.Do < 1 || a.Ho < 1 || a.Wo < 1 || a.B < 1) return false;
    const long long last = (b.Cout - 1) * b.oc + (a3 ? (b.Do - 1) * b.od : 0) + (b.Ho - 1) * b.oh + b.Wo;
    if (4 * last >= static_cast<long long>(kOOB) || b.oc >= (1 << 28) || b.od >= (1 << 28) || b.oh >= (1 << 28)) return false;
    return pk_geo(a, b, a3, 1, nullptr) <= kPkMaxLds;
}

// What a K-split launch of a pair pairk_ok accepted cannot run: a grid past the limits at its tile rows
int pairk_tile_check(const esm_conv_desc& a, const esm_conv_desc& b) {
    if (ceil_div(b.Ho, pk_rows(a, b)) > 65535 || static_cast<long long>(b.Do) * a.B > 65535)
        return arg_error("conv pair (K-split): grid too large");
    return ESM_OK;
}

// a, b: a pair pair2_form named ESM_PAIR_FORM_KSPLIT
int launch_pairk(const esm_conv_desc& a, const esm_conv_desc& b, hipStream_t s) {
    const bool d3 = a.kd > 1;
    const bool mt2 = a.Cout > 16 || b.Cout > 16;
#define ESM_PK(D, S) (mt2 ? launch_pk<D, S, 2>(a, b, s) : launch_pk<D, S, 1>(a, b, s))
    if (d3) return a.stride == 2 ? ESM_PK(true, 2) : ESM_PK(true, 1);
    return a.stride == 2 ? ESM_PK(false, 2) : ESM_PK(false, 1);
#undef ESM_PK
}

}  // namespace conv
}  // namespace esm
