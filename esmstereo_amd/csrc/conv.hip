// esm_conv_f32: descriptor validation (host side, before anything touches the GPU) and
// dispatch to the 2-D / 3-D implicit-GEMM instantiations (conv2d.hip, conv3d.hip).
#include "conv_c1_rec.h"
#include "conv_lean_rec.h"

namespace esm {

int launch_conv2d(const esm_conv_desc& a, hipStream_t s);
int launch_conv3d(const esm_conv_desc& a, hipStream_t s);
namespace conv {
bool stem_ok(const esm_conv_desc& a);                    // conv_stem.hip
bool stem_auto(const esm_conv_desc& a);                  // conv_stem.hip
int launch_stem(const esm_conv_desc& a, hipStream_t s);  // conv_stem.hip
bool c1in_ok(const esm_conv_desc& a);                    // conv_stem.hip
int launch_c1in(const esm_conv_desc& a, hipStream_t s);  // conv_stem.hip
bool small_ok(const esm_conv_desc& a);                   // conv_small.hip
bool small_auto(const esm_conv_desc& a);                 // conv_small.hip
bool lean_record(const esm_conv_desc& a, unsigned (&rec)[kLeanRecDwords]);  // conv_small.hip
int launch_small(const esm_conv_desc& a, hipStream_t s);  // conv_small.hip
bool wide_ok(const esm_conv_desc& a);                    // conv_wide.hip
int launch_wide(const esm_conv_desc& a, hipStream_t s);  // conv_wide.hip
bool wide3_ok(const esm_conv_desc& a);                    // conv_wide3.hip
int launch_wide3(const esm_conv_desc& a, hipStream_t s);  // conv_wide3.hip
bool widet_ok(const esm_conv_desc& a);                    // conv_widet.hip
int launch_widet(const esm_conv_desc& a, hipStream_t s);  // conv_widet.hip
bool tile3_auto(const esm_conv_desc& a);                 // conv_tile3.hip
int launch_tile3(const esm_conv_desc& a, hipStream_t s);  // conv_tile3.hip
bool tile2_auto(const esm_conv_desc& a);                 // conv_tile3.hip
bool tile2_ok(const esm_conv_desc& a);                   // conv_tile3.hip
int launch_tile2(const esm_conv_desc& a, hipStream_t s);  // conv_tile3.hip
bool pw_ok(const esm_conv_desc& a);                       // conv_pw.hip
bool pw_auto(const esm_conv_desc& a);                     // conv_pw.hip
int launch_pw(const esm_conv_desc& a, hipStream_t s);     // conv_pw.hip
}  // namespace conv

// Descriptor validation shared by every entry point that takes an esm_conv_desc (launch_conv, the
// chain of chain.hip); ESM_OK or ESM_ERR_ARG with the message set.
int conv_check(const esm_conv_desc& a) {
    if (!a.w || !a.out) return arg_error("conv: null weights/output");
    if (a.nsrc < 1 || a.nsrc > ESM_MAX_SRC) return arg_error("conv: nsrc must be 1..3");
    int cin = 0;
    for (int i = 0; i < ESM_MAX_SRC; ++i) {
        if (i < a.nsrc) {
            if (!a.src[i].ptr || a.src[i].C <= 0) return arg_error("conv: bad source");
            cin += a.src[i].C;
        } else if (a.src[i].C != 0) {
            return arg_error("conv: unused source slots must have C = 0");
        }
    }
    if (cin != a.Cin) return arg_error("conv: Cin != sum of source channels");
    if (a.B <= 0 || a.Cout <= 0) return arg_error("conv: bad B/Cout");
    if (a.cin_pad % 16 || a.cin_pad < a.Cin) return arg_error("conv: cin_pad must be a multiple of 16 >= Cin");
    if (a.cout_pad % 32 || a.cout_pad < a.Cout) return arg_error("conv: cout_pad must be a multiple of 32 >= Cout");
    const bool d3 = is3d(a);
    if (a.kh != a.kw) return arg_error("conv: kh must equal kw");
    if (d3 && a.kd != a.kh) return arg_error("conv: 3-D kernels must be cubic");
    if (!d3 && (a.Di != 1 || a.Do != 1)) return arg_error("conv: 2-D conv needs Di = Do = 1");
    if (a.shuffle > 1 && (d3 || a.transposed)) return arg_error("conv: pixel shuffle only for 2-D convs");
    if (a.up && (a.Cout != 1 || d3 || a.up_f <= 0)) return arg_error("conv: bilinear add needs 2-D, Cout == 1");
    if (a.Hi <= 0 || a.Wi <= 0 || a.Di <= 0) return arg_error("conv: empty input");
    // No form addresses an operand whose offset within one channel (its planes and rows) reaches 2^31 elements:
    // the LDS-staged general form, the last resort of every 32-bit form's guard, narrows a source's (plane, row)
    // offset to int (conv_impl.h load_chunk).  Refused for every operand, so that what a layer accepts as its
    // input it also accepts as a predecessor's output.
    {
        constexpr long long kPlaneMax = 1LL << 31;
        auto past = [&](long long planes, int64_t sd, long long rows, int64_t sh, long long cols) {
            const int64_t pd = planes > 1 ? sd : 0;
            // (a stride of that size alone, in either direction; and the sum below cannot overflow)
            if (pd >= kPlaneMax || sh >= kPlaneMax || pd <= -kPlaneMax || sh <= -kPlaneMax) return true;
            return (planes - 1) * pd + (rows - 1) * sh + cols >= kPlaneMax;
        };
        const long long r = a.shuffle > 1 ? a.shuffle : 1;
        const long long d_out = d3 ? a.Do : 1, h_out = a.Ho * r, w_out = a.Wo * r;
        bool bad = a.Ho > 0 && a.Wo > 0 && a.Do > 0 && past(d_out, a.od, h_out, a.oh, w_out);  // out, out2
        for (int i = 0; i < a.nsrc; ++i) bad = bad || past(d3 ? a.Di : 1, a.src[i].sd, a.Hi, a.src[i].sh, a.Wi);
        if (a.res && a.Ho > 0 && a.Wo > 0 && a.Do > 0) bad = bad || past(d_out, a.rd, h_out, a.rh, w_out);
        if (a.mul && a.Ho > 0 && a.Wo > 0) bad = bad || past(1, 0, a.Ho, a.mh, a.Wo);
        if (a.up && a.up_h > 0 && a.up_w > 0) bad = bad || past(1, 0, a.up_h, a.uh, a.up_w);
        if (bad) return arg_error("conv: an operand's offset within one channel reaches 2^31 elements");
    }
    // the packed weights [taps][cin_pad][cout_pad]: every form that reads them through a buffer descriptor takes
    // 32-bit byte offsets (out-of-range marks at 1 GiB)
    if (static_cast<long long>(a.kd > 0 ? a.kd : 1) * a.kh * a.kw * a.cin_pad * a.cout_pad * 4 >= (1LL << 30))
        return arg_error("conv: packed weights of 1 GiB or more");
    if (a.transposed) {
        if (a.kh != 4 || a.stride != 2 || a.ph != 1 || a.pw != 1 || (d3 && a.pd != 1))
            return arg_error("conv: transposed conv supports k=4, s=2, p=1 only");
        if (a.Ho != 2 * a.Hi || a.Wo != 2 * a.Wi || (d3 && a.Do != 2 * a.Di))
            return arg_error("conv: transposed output extent must be 2x the input");
        return ESM_OK;
    }
    const int S = a.stride;
    if (S != 1 && S != 2) return arg_error("conv: stride must be 1 or 2");
    if (a.Ho != (a.Hi + 2 * a.ph - a.kh) / S + 1 || a.Wo != (a.Wi + 2 * a.pw - a.kw) / S + 1 ||
        (d3 && a.Do != (a.Di + 2 * a.pd - a.kd) / S + 1))
        return arg_error("conv: output extent inconsistent with kernel/stride/padding");
    if (a.Ho <= 0 || a.Wo <= 0 || a.Do <= 0) return arg_error("conv: empty output");
    return ESM_OK;
}

// The form a (checked) descriptor takes: an ESM_FORM_* value, or ESM_ERR_ARG with the message set.  The rules
// of every round, in the order they were measured in; launch_conv switches over the result and esm_conv_form
// reports it.  A forced form (hint) is returned as forced: whether it runs the layer is its launcher's check,
// except for the two forms that step aside for the automatic rules (wide, pointwise).  *hint: the hint the
// chosen form's launcher gets (a wide hint that stepped aside, and NO_STEM, are consumed here).
int select_form(const esm_conv_desc& a, int* hint) {
    *hint = a.hint;
    const bool d3 = is3d(a);
    const int tile = d3 ? ESM_FORM_TILE3 : ESM_FORM_TILE2;
    const int form = a.hint & ~(ESM_HINT_XCD_SLAB | ESM_HINT_NO_TILE);  // the form / tile bits
    const bool tile_auto = form == 0 && !(a.hint & ESM_HINT_NO_TILE);
    if (a.transposed) {
        if (a.hint & ESM_HINT_WIDET) return ESM_FORM_WIDET;
        if (a.hint & ESM_HINT_TILE) return tile;
        // large maps (L at B = 4: ref4x.conv2_up 103 -> 61 us, r04 probe): the LDS-tiled form
        if (tile_auto && (d3 ? conv::tile3_auto(a) : conv::tile2_auto(a))) return tile;
        if ((a.hint & ESM_HINT_SMALL) || (form == 0 && conv::small_auto(a))) return ESM_FORM_SMALL;
        return ESM_FORM_GENERAL;
    }
    // 1x1 on the large maps / volumes: the pointwise streaming form (round 6); TILE | TILE_PW forces it, TILE
    // alone the LDS-tiled k1 form (A/B)
    if (((a.hint & ESM_HINT_TILE) && (a.hint & ESM_HINT_TILE_PW)) || (tile_auto && conv::pw_auto(a))) {
        if (conv::pw_ok(a)) return ESM_FORM_PW;
    }
    if (a.hint & ESM_HINT_SMALL) return ESM_FORM_SMALL;
    if (a.hint & ESM_HINT_WIDE) {
        // a tuned choice for a layer the wide form cannot take after all (concat sources with different
        // row strides, e.g. a cropped view): the automatic rules instead
        if (conv::wide_ok(a)) return ESM_FORM_WIDE;
        esm_conv_desc d = a;
        d.hint &= ESM_HINT_XCD_SLAB;
        return select_form(d, hint);
    }
    if (a.hint & ESM_HINT_WIDE3) return ESM_FORM_WIDE3;
    if (a.hint & ESM_HINT_TILE) return tile;
    // the MFMA-bound 3-D volumes / 2-D maps of ESMStereo-L / -M: the LDS-tiled form
    if (tile_auto && (d3 ? conv::tile3_auto(a) : conv::tile2_auto(a))) return tile;
    if (a.hint & ESM_HINT_STEM) return ESM_FORM_STEM;
    if (a.hint & ESM_HINT_C1IN) return ESM_FORM_C1IN;
    // one input channel, 2-D, large map: the VALU form (an MFMA k-step would be 3/4 padding).
    // Measured (scripts/probes/c1in_sweep.py, profiles/r01_c1in_sweep.txt): 1->16 k3s2 at 192x624
    // output 8.6 us; on small maps the MFMA direct form wins (4.8 vs 11.6 us at 24x78)
    if (form == 0 && conv::c1in_ok(a) && static_cast<long long>(a.B) * a.Ho * a.Wo >= 65536)
        return ESM_FORM_C1IN;
    if (a.hint & ESM_HINT_NO_STEM) {
        *hint = a.hint & ~ESM_HINT_NO_STEM;
        return ESM_FORM_GENERAL;
    }
    // 8 / 12 / 24 output channels, 3x3(x3) stride 1: the 16-block MFMA form wastes no tile rows
    if (form == 0 && conv::stem_auto(a)) return ESM_FORM_STEM;
    // latency-bound layers (most of the hot path): the lean K-split form (conv_small.hip)
    if (form == 0 && conv::small_auto(a)) return ESM_FORM_SMALL;
    return ESM_FORM_GENERAL;
}

int conv_form(const esm_conv_desc* d, int* hint) {
    if (!d) return arg_error("conv: null descriptor");
    const int rc = conv_check(*d);
    return rc != ESM_OK ? rc : select_form(*d, hint);
}

int launch_conv(const esm_conv_desc* d, hipStream_t s) {
    int hint = 0;
    const int form = conv_form(d, &hint);
    if (form < 0) return form;
    esm_conv_desc a = *d;
    a.hint = hint;
    switch (form) {
        case ESM_FORM_STEM: return conv::launch_stem(a, s);
        case ESM_FORM_C1IN: return conv::launch_c1in(a, s);
        case ESM_FORM_SMALL: return conv::launch_small(a, s);
        case ESM_FORM_WIDE: return conv::launch_wide(a, s);
        case ESM_FORM_WIDE3: return conv::launch_wide3(a, s);
        case ESM_FORM_WIDET: return conv::launch_widet(a, s);
        case ESM_FORM_TILE3: return conv::launch_tile3(a, s);
        case ESM_FORM_TILE2: return conv::launch_tile2(a, s);
        case ESM_FORM_PW: return conv::launch_pw(a, s);
        default: break;
    }
    return is3d(a) ? launch_conv3d(a, s) : launch_conv2d(a, s);
}

}  // namespace esm

extern "C" int esm_conv_f32(const esm_conv_desc* desc, void* stream) {
    return esm::launch_conv(desc, esm::as_stream(stream));
}

extern "C" int esm_lean_record_pack(const esm_conv_desc* desc, uint32_t rec[14], int64_t fields[19]) {
    if (!desc || !rec || !fields) return esm::arg_error("lean_record_pack: null argument");
    unsigned d[esm::conv::kLeanRecDwords];
    if (!esm::conv::lean_record(*desc, d)) return 0;
    const esm::conv::LeanRec r = esm::conv::lean_record_unpack(d);
    const int64_t f[19] = {r.sb, r.sc, r.sd, r.sh, r.m_ds, r.m_b, r.Wi, r.Hi, r.Di, r.Ws, r.Ds, r.B, r.Cin, r.cout_pad,
                           r.pd, r.ph, r.pw, r.xcd, r.has_scale};
    return esm::conv::record_export(d, f, rec, fields);
}

extern "C" int esm_c1_record_pack(const esm_conv_desc* desc, const uint32_t grid[3], uint32_t rec[16], int64_t fields[16]) {
    if (!desc || !grid || !rec || !fields) return esm::arg_error("c1_record_pack: null argument");
    unsigned d[esm::conv::kC1RecDwords];
    esm::conv::c1_record_pack(*desc, dim3(grid[0], grid[1], grid[2]), d);
    const esm::conv::C1Rec r = esm::conv::c1_record_unpack(d);
    const int64_t f[16] = {esm::conv::ptr_field(r.src), esm::conv::ptr_field(r.w), r.sb, r.sc, r.sh, r.Hi, r.Wi, r.Cin,
                           r.cin_pad, r.cout_pad, r.slab, r.gx, r.gy, r.nwg, r.m_gx, r.m_gy};
    return esm::conv::record_export(d, f, rec, fields);
}

extern "C" int esm_c1_record_tile(const uint32_t rec[16], uint32_t bx, uint32_t by, uint32_t bz, int32_t xyz[3]) {
    if (!rec || !xyz) return esm::arg_error("c1_record_tile: null argument");
    unsigned d[esm::conv::kC1RecDwords];
    for (int i = 0; i < esm::conv::kC1RecDwords; ++i) d[i] = rec[i];
    const esm::Blk3 t = esm::conv::c1_tile(esm::conv::c1_record_unpack(d), bx, by, bz);
    xyz[0] = t.x, xyz[1] = t.y, xyz[2] = t.z;
    return 1;
}

extern "C" int esm_conv_form(const esm_conv_desc* desc) {
    int hint = 0;
    return esm::conv_form(desc, &hint);
}
