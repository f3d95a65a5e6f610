/*
 * esmstereo_amd — C ABI of the MI355X (gfx950) ESMStereo hot path.
 *
 * Every entry point takes caller-owned DEVICE pointers (fp32, contiguous unless a stride
 * is given), plain sizes and a HIP stream handle passed as `void*` (a `hipStream_t`; NULL =
 * the default stream).  Kernels never allocate or free; launches are stream-ordered and the
 * library keeps no global mutable state apart from a thread-local last-error string.
 * Return value: ESM_OK (0) or a negative ESM_ERR_* code; esm_last_error() says why.
 *
 * Each function replaces one reference interface (file:line in /root/reference):
 *   esm_gwc_volume_f32        models/submodule.py:151-161 build_gwc_volume (+ the S-variant
 *                             `volume * att` at models/ESMStereo.py:711 when att != NULL)
 *   esm_concat_volume_f32     models/submodule.py:129-140 build_concat_volume
 *   esm_normcorr_volume_f32   models/submodule.py:187-200 build_norm_correlation_volume
 *   esm_disp_regression_f32   models/submodule.py:211-216 disparity_regression
 *   esm_topk2_regression_f32  models/submodule.py:218-225 regression_topk(cost, arange, k=2)
 *   esm_topk_regression_f32   models/submodule.py:218-225 regression_topk(cost, samples, k), any k
 *   esm_conv_f32              models/submodule.py:12-38 BasicConv (Conv2d/3d, ConvTranspose2d/3d,
 *                             eval BatchNorm, GELU) and the plain convs of models/ESMStereo.py:
 *                             129-509 with their fused neighbours (crop+cat :172,177,230,234;
 *                             PixelShuffle+SiLU :265-268; bilinear-upsample + add :307,316;
 *                             `* att` :703; residual adds of models/shufflemixer.py:130-131)
 *   esm_fmnet_f32             models/shufflemixer.py:100-112,129-130 FMBlock.net (two SMLayers) + x
 *   esm_smix_f32              models/shufflemixer.py:23-112 LayerNorm('BiasFree') +
 *                             SplitPointMlp + channel shuffle + residual, optionally preceded
 *                             by the depthwise 7x7 `spatial` conv
 *   esm_shuffle_tail_f32      models/ESMStereo.py:264-271,290-302,311-312 (and the upsample8 /
 *                             upsample16 twins): `upsampling` (Conv2d 1x1 nf -> nf*r*r + bias,
 *                             PixelShuffle(r), SiLU) followed by `tail` (Conv2d 3x3 nf -> 1 +
 *                             bias) as one kernel; the shuffled map is never materialised
 *   esm_shuffle_conv_f32      the same head followed by up_refinement.conv1[0] (models/ESMStereo.py:
 *                             190-191, the refinement's first BasicConv(1, C, 3, 2, 1)) in one kernel
 *   esm_conf_f32              the per-pixel stages of the confidence head LAFNet_ESM /
 *                             conf_upsample (models/ESMStereo_confidence.py:511-744) between its
 *                             convs (which run through esm_conv_f32): cost features, attention,
 *                             the scale-driven 3x grid_sample, the softmax-weighted x4 upsample
 *   esm_plan_*                the orchestration of models/ESMStereo.py:700-745 as a native
 *                             launch list, optionally replayed as one hipGraph
 *   esm_preprocess_u8         the input side: pad to /32 + ToTensor +
 *                             Normalize of test_kitti.py:93-106 (pad before normalising) or
 *                             datasets/kitti_dataset.py:151-170 (pad after), datasets/data_io.py:7-16
 *   esm_node_filter_u16       the ROS node's post-processing (kitti_publisher_cuda_node.cpp:385-403):
 *                             crop, medianBlur 5x5, valid mask, x256 -> uint16
 *   esm_disp_to_u16           the output side: crop of the padded disparity (test_kitti.py:115,
 *                             save_disp.py:81) + np.round(d * 256).astype(np.uint16) (save_disp.py:85)
 *   esm_disp_metrics_f32      utils/metrics.py:17-74 EPE_metric / D1_metric / D1_metric_thres / Thres_metric
 *                             (train_kitti.py:221-232, train_sceneflow.py:239-250) and the host-side EPE and
 *                             bad-pixel rates of test_kitti.py:117-125, test_eth3d.py:93-98, test_mid.py:106-114
 *   esm_disp_metrics_workspace  the size of the scratch buffer esm_disp_metrics_f32 takes
 *   esm_disp_error_map_f32    utils/visualization.py:20-37 vis (test_kitti.py:134)
 *   esm_disp_colorize_u8      the colour-mapped frame: save_vid.py:118-125, save_disp.py:87-97, test_mid.py:118-121,
 *                             test_eth3d.py:102-105 (convertScaleAbs + applyColorMap, stacked under the left image),
 *                             kitti_publisher_cuda_node.cpp:81-86,117-118 (minMaxLoc, convertTo, applyColorMap,
 *                             vconcat), latest.py:60-64 (depth colour map)
 *   esm_disp_colorize_workspace  the size of the scratch buffer esm_disp_colorize_u8 takes in RANGE mode
 *   esm_disp_to_depth_f32     latest.py:56-57 depth = baseline * focal / disparity, clipped to [0, max_depth]
 *   esm_node_filter_conf_u16  the confidence-gated node's post-processing (kitti_publisher_conf_cuda_node.cpp:
 *                             555-576): esm_node_filter_u16 with conf >= threshold in the valid mask
 *   esm_node_panels_u8        its four-panel frame (:183-257 without the overlays): left image, colour-mapped
 *                             disparity, the node's error map (:69-151) and the confidence map
 *   esm_depth16_to_disp_f32   virtual_kitti_publisher_cuda_node.cpp:55-77,146-147: ground-truth disparity from a
 *                             16-bit depth image, resized (INTER_LINEAR) to the network size
 *   esm_resize_u8             virtual_kitti_publisher_cuda_node.cpp:186-188,211-213: cv::resize(..., INTER_LINEAR) of
 *                             an 8-bit image (the left image at the network size; the stacked picture's squeeze)
 *   esm_preprocess_resize_u8  virtual_kitti_publisher_cuda_node.cpp:232-266, kitti_publisher_ess_cuda_node.cpp:241-275
 *                             preprocess_image: resize to the network size, /255, mean and std, planar fp32
 */
#ifndef ESMSTEREO_AMD_H
#define ESMSTEREO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ESM_OK 0
#define ESM_ERR_ARG (-1)
#define ESM_ERR_LAUNCH (-2)
#define ESM_ERR_UNSUPPORTED (-3)
#define ESM_ERR_RUNTIME (-4)

#define ESM_ACT_NONE 0
#define ESM_ACT_GELU 1 /* exact erf GELU, nn.GELU() */
#define ESM_ACT_SILU 2
#define ESM_ACT_RELU 3
#define ESM_ACT_SIGMOID 4 /* 1 / (1 + exp(-x)), torch.sigmoid */
#define ESM_ACT_RELU6 5   /* min(max(x, 0), 6), nn.ReLU6 (the MobileNetV2 backbone) */

#define ESM_MAX_SRC 3

/* One channel-slice source of a (possibly concatenated, possibly cropped) conv input.
 * Element strides; the innermost (W) stride is 1.  For 2-D tensors sd is ignored. */
typedef struct {
    const float* ptr;
    int32_t C;
    int32_t reserved;
    int64_t sb, sc, sd, sh;
} esm_src;

/* esm_conv_desc.hint: 0 = the automatic choice, else one form selector | that form's fields.  XCD_SLAB
 * goes with any value, 0 included.  This table is the definition; every reader uses these names.
 *
 *   selector   form (launcher)                                fields it reads
 *   (none)     general: direct / LDS-staged / row-streaming   NT | KS | C1 | DIRECT | ROWS_FORM | RPW: an explicit tile
 *   C1T        VALU single-output ConvTranspose (conv_c1.h)    ROWS(1): 3-D per-class form (A/B)
 *   STEM       16-block narrow-output form (conv_stem.hip)     -
 *   NO_STEM    automatic, without STEM                         -
 *   NO_TILE    automatic, without the LDS-tiled forms (A/B)    -
 *   C1IN       VALU single-input-channel form (conv_stem.hip)  -
 *   SMALL      lean K-split form (conv_small.hip)              SMALL_W8, SMALL_NO_ZSPLIT, SMALL_NO_RECORD
 *   WIDE       register-weight row-streaming (conv_wide.hip)   ROWS(1 / 2 / 3) = 2 / 4 / 8 rows per wave, WIDE_KS2
 *   TILE       LDS-tiled implicit GEMM (conv_tile3.hip)        ROWS(1 / 2 / 3) = 1 / 2 / 4 rows per wave; TILE_PW on a
 *                                                              1x1; on a 3x3x3: TILE_WLDS, TILE_DMA_FLIP, TILE_ROWS8
 *   WIDE3      register-weight 3x3x3 form (conv_wide3.hip)     -
 *   WIDET      register-weight ConvTranspose2d (conv_widet.hip) ROWS(1 / 2) = 1 / 2 sub-grid rows per wave
 *
 * Outside esm_conv_f32: esm_gwc_stem_f32 reads ROWS(2 / 3) = 2 / 4 rows per wave and GWC_STEM_WLDS of stem->hint;
 * esm_conv_pair2_f32 reads PAIR_REGRESS of a->hint and ROWS, PAIRK, PAIR_NO_RECORD of b->hint (see there); esm_convt_1x1_f32 reads
 * TILE, SMALL and ROWS(1 / 2) of a->hint.  ROWS(0) is always the form's automatic choice. */
#define ESM_HINT_NT_MASK 0xF         /* general form: N tiles per wave, 1 / 2 / 4 */
#define ESM_HINT_KS_SHIFT 4          /* general form: K split, 1 / 4 */
#define ESM_HINT_KS_MASK (0xF << 4)
#define ESM_HINT_C1 (1 << 8)         /* general form: VALU path for <= 2 couts (NT 4, KS 1) */
#define ESM_HINT_SMALL_NO_RECORD (1 << 8) /* SMALL (the bit is the general form's C1 otherwise): the struct-argument kernel
                                             even where the first-load record describes the layer (A/B, tests) */
#define ESM_HINT_DIRECT (1 << 9)     /* general form: direct (register-operand) variant */
#define ESM_HINT_ROWS_FORM (1 << 10) /* general form: row-streaming variant (conv_rows.h) */
#define ESM_HINT_RPW_SHIFT 12        /* DIRECT: rows per wave, 0 = automatic */
#define ESM_HINT_RPW_MASK (0xF << 12)
#define ESM_HINT_C1T (1 << 16)
#define ESM_HINT_STEM (1 << 17)
#define ESM_HINT_NO_STEM (1 << 18)
#define ESM_HINT_NO_TILE (1 << 19)
#define ESM_HINT_C1IN (1 << 20)
#define ESM_HINT_SMALL (1 << 21)
#define ESM_HINT_WIDE (1 << 22)
#define ESM_HINT_TILE (1 << 23)
#define ESM_HINT_WIDE3 (1 << 24)
#define ESM_HINT_WIDET (1 << 25)
#define ESM_HINT_ROWS_SHIFT 26
#define ESM_HINT_ROWS_MASK (3 << 26)
#define ESM_HINT_ROWS(n) ((n) << 26)
/* bit 28, by reader */
#define ESM_HINT_WIDE_KS2 (1 << 28)      /* WIDE: each strip's channel groups over two waves (>= 2 groups, >= 4 rows) */
#define ESM_HINT_TILE_DMA_FLIP (1 << 28) /* TILE 3x3x3, s2 <= 32 couts or s1 <= 8 couts: input window through registers,
                                            not buffer-to-LDS; s1 24 / 40 couts: the other staging (24: DMA, 40: not) */
#define ESM_HINT_TILE_ROWS8 (1 << 28)    /* TILE 3x3x3 s1, other couts, with ROWS(3): 8 rows per wave */
#define ESM_HINT_PAIRK (1 << 28)         /* pair2 b->hint: the K-split form (conv_pairk.hip) */
#define ESM_HINT_GWC_STEM_WLDS (1 << 28) /* gwc_stem: composite weights staged in LDS, not registers */
#define ESM_HINT_SMALL_NO_ZSPLIT (1 << 28) /* SMALL 3x3x3, <= 6 channel groups: each wave walks a group's 27 taps, not
                                              one (group, tap plane) unit of 9 (A/B) */
/* bit 29, by reader */
#define ESM_HINT_SMALL_W8 (1 << 29)      /* SMALL: 8 waves per workgroup splitting K (> 4 channel groups) */
#define ESM_HINT_TILE_PW (1 << 29)       /* TILE on a 1x1: the pointwise streaming form (conv_pw.hip) where it fits */
#define ESM_HINT_TILE_WLDS (1 << 29)     /* TILE 3x3x3: weights staged in LDS (s2; s1 <= 8 couts), padded MT (24, 40) */
#define ESM_HINT_PAIR_REGRESS (1 << 29)  /* pair2 a->hint: a's input is disparity_regression of src[0] (see there) */
#define ESM_HINT_PAIR_NO_RECORD (1 << 29) /* pair2 b->hint, LDS form: the struct-argument kernel even where the staging
                                             record describes the pair (A/B, tests) */
#define ESM_HINT_XCD_SLAB (1 << 30) /* tile order: each XCD runs a contiguous band of tiles, so halo rows are fetched
                                       once per band (small / wide / wide3 / wideT / tiled / pair / C1T / gwc_stem) */

/* Implicit-GEMM convolution on NC(D)HW fp32, fp32 MFMA.
 * 2-D convs use kd = 1, Di = Do = 1.
 * Transposed convs are supported for kernel 4, stride 2, padding 1 (the only form the
 * reference uses); out extent = 2 x in extent.
 * Supported (kernel, stride) of the other convs, any padding: 2-D (1, 1), (3, 1), (3, 2), (5, 1); 3-D (1, 1),
 *   (3, 1), (3, 2).  Any other pair passes validation and esm_conv_f32 returns ESM_ERR_UNSUPPORTED for it at
 *   every size; esm_conv_form answers for the supported geometry only (it reports ESM_FORM_GENERAL for the rest).
 * weights: packed by esm_conv_pack_* conventions (see esmstereo_amd/engine.py):
 *   normal:     w[tap][cin_pad][cout_pad], tap = (kd_i*kh + kh_i)*kw + kw_i
 *   transposed: w[cls][tap][cin_pad][cout_pad], cls = parity class of the output voxel
 * Epilogue order: v = acc*scale[c] + shift[c] (scale NULL -> 1, shift NULL -> 0);
 *   v = act(v); v *= mul[b,c,y,x] (broadcast over d); v += res[b,c,d,y,x];
 *   v = bilinear_up(up)[b,0,y,x] + v; store v * post_scale (through a PixelShuffle of
 *   factor `shuffle` when > 1) and, when out2 != NULL, v * post_scale2 to out2. */
typedef struct {
    esm_src src[ESM_MAX_SRC];
    int32_t nsrc;
    int32_t B, Cin;
    int32_t Di, Hi, Wi;
    int32_t Do, Ho, Wo;
    int32_t kd, kh, kw;
    int32_t stride;
    int32_t transposed;
    int32_t pd, ph, pw;
    int32_t Cout;
    int32_t cin_pad, cout_pad;
    const float* w;
    const float* scale;
    const float* shift;
    int32_t act;
    int32_t shuffle;
    const float* mul;
    int64_t mb, mc, mh;
    const float* res;
    int64_t rb, rc, rd, rh;
    float* out;
    int64_t ob, oc, od, oh;
    const float* up;
    int32_t up_h, up_w, up_f;
    int32_t hint; /* 0 = automatic; else ESM_HINT_* bits (the table above esm_conv_desc) */
    int64_t ub, uh;
    float post_scale;
    float post_scale2;
    float* out2; /* nullable: second copy of the result (same strides as out), x post_scale2 / post_scale */
} esm_conv_desc;

/* ShuffleMixer per-pixel chain on a [B, C, H, W] tensor, C in {8, 16}:
 *   t = dw ? (depthwise KxK conv of x with bias) : x          (SMLayer.spatial)
 *   for s in stages: t = shuffle(cat(fc2(silu(fc0(LN_s(t)[:C/2]))), LN_s(t)[C/2:])) + t
 *   if res: t += res
 * (SMLayer.forward, shufflemixer.py:108-112; FMBlock `net(x) + x`, :130). */
#define ESM_SMIX_MAX_STAGES 2
typedef struct {
    const float* ln_w;  /* [C] */
    const float* fc0_w; /* [C][C/2] */
    const float* fc0_b; /* [C] */
    const float* fc2_w; /* [C/2][C] */
    const float* fc2_b; /* [C/2] */
} esm_smix_stage;

typedef struct {
    const float* x;
    float* out;
    const float* res; /* nullable */
    const float* dw_w; /* [C][K][K], nullable (no depthwise) */
    const float* dw_b; /* [C] */
    int32_t dw_k;
    int32_t nstages;
    esm_smix_stage stage[ESM_SMIX_MAX_STAGES];
    int32_t B, C, H, W;
} esm_smix_desc;

/* The whole `net` of an FMBlock (two SMLayers, models/shufflemixer.py:100-112,129-130) in one launch:
 * out = SMLayer1(SMLayer0(x)) + x, where SMLayer(t) = mlp2(dw(mlp1(t))) with mlp = the per-pixel
 * LN -> SplitPointMlp -> shuffle -> residual chain of esm_smix_desc.  stage[] = SMLayer0.mlp1,
 * SMLayer0.mlp2, SMLayer1.mlp1, SMLayer1.mlp2; dw_w/dw_b[l] = SMLayer l's depthwise K x K conv
 * (K = 7); C in {8, 16}.  The three esm_smix_f32 launches it replaces, in one (same operations). */
typedef struct {
    const float* x;
    float* out;
    const float* dw_w[2];
    const float* dw_b[2];
    int32_t dw_k;
    int32_t reserved;
    esm_smix_stage stage[4];
    int32_t B, C, H, W;
    /* optional, conv0_w != NULL: FMBlock.conv fused behind net (shufflemixer.py:124-131), out =
     * conv2(silu(conv0(t) + conv0_b)) + conv2_b + t with t = net(x) + x; conv0_w [hid][C][3][3] (zero
     * padding 1), conv0_w/b [hid], conv2_w [C][hid], conv2_b [C]; hid = C + 16 */
    const float* conv0_w;
    const float* conv0_b;
    const float* conv2_w;
    const float* conv2_b;
    int32_t hid;
    int32_t reserved2;
    /* optional, with conv0_w: a [B, C, H, W] scratch buffer; when given, the block runs as two launches
     * split at the second depthwise conv (halo 3 each side instead of the whole block's 7) with FMBlock.conv
     * on the matrix cores: the form for large maps (ESMStereo-L at KITTI size and up) */
    float* work;
} esm_fmnet_desc;

/* Fused `tail(upsampling(x))` of the ESM upsamplers: out[b,0] = tail_b + conv3x3(tail_w,
 * silu(pixel_shuffle(conv1x1(up_w, x) + up_b, r))), zero padding 1.  (nf, r) in
 * {(8,2), (8,4), (16,2), (16,4)}.  x: [B, nf, H, W] with strides xb, xc, xh (innermost 1);
 * out: [B, 1, r*H, r*W] with strides ob, oh.  tail_b may be NULL (no bias). */
typedef struct {
    const float* x;
    int64_t xb, xc, xh;
    const float* up_w;   /* [nf*r*r][nf] */
    const float* up_b;   /* [nf*r*r] */
    const float* tail_w; /* [nf][3][3] */
    const float* tail_b; /* [1] or NULL */
    float* out;
    int64_t ob, oh;
    int32_t B, nf, H, W, r;
    int32_t flags; /* bit 0: XCD-slab tile order (each XCD runs a contiguous band of output rows; see
                      ESM_HINT_XCD_SLAB); bits 1-2, (nf, r) = (8, 4) only: 0 automatic, 1 the
                      low-res-window form, 2 / 3 the MFMA row form with 4 / 8 low-res rows per workgroup */
} esm_shuffle_tail_desc;

/* `tail(upsampling(x))` (as esm_shuffle_tail_desc, st.out unused) followed by the refinement
 * hourglass's first layer BasicConv(1, C, 3, stride 2, pad 1) + folded BN + exact GELU
 * (up_refinement.conv1[0], models/ESMStereo.py:190-191), in one launch; the 1-channel map between
 * them is never stored.  w: packed conv weights [9][cin_pad][cout_pad] (cin 1); scale/shift: the
 * folded BN (scale NULL = 1); out: [B, C, ceil(r*H/2), ceil(r*W/2)] with strides ob, oc, oh.
 * (nf, r, C) in {(8, 4, 16), (8, 2, 16), (16, 2, 32), (16, 4, 32)}.  st.flags bit 0: XCD-slab tile order;
 * bits 1-2, (8, 4, 16) only: 0 automatic, 1 the low-res-window form, 2 the MFMA row form (8 low-res rows
 * per workgroup), 3 the same row form with the refinement conv on the matrix cores. */
typedef struct {
    esm_shuffle_tail_desc st;
    const float* w;
    const float* scale;
    const float* shift;
    float* out;
    int64_t ob, oc, oh;
    int32_t C, cin_pad, cout_pad, reserved;
    /* Optional pre-conv (nf 8, r 4, C 16 row form only): with pre_x set, the head's input x is not read from
     * st.x (which must be NULL) but computed in the launch as GELU(BN(Conv2d(pre_cin, nf, 3, 1, 1)(pre_x)))
     * -- the upsampler stage's spx_<t>[1] (models/ESMStereo.py:247-259) -- from pre_x [B, pre_cin, H, W]
     * (strides pb, pc, ph; pre_cin <= 16), packed weights pre_w [9][pre_cin_pad][pre_cout_pad] and the
     * folded BN pre_scale / pre_shift (pre_scale NULL = 1). */
    const float* pre_x;
    int64_t pb, pc, ph;
    const float* pre_w;
    const float* pre_scale;
    const float* pre_shift;
    int32_t pre_cin, pre_cin_pad, pre_cout_pad, pre_reserved;
    /* Optional second conv (nf 8, r 4, C 16 row form with pre_x only): with w2 set, the refinement's
     * conv1[1] (BasicConv(C, C, 3, 1, 1): folded BN scale2 / shift2 (scale2 NULL = 1) + exact GELU, packed
     * w2 [9][cin_pad2][cout_pad2]) runs in the same launch on the first conv's map, which is never stored:
     * `out` receives conv1[1]'s output (same shape and strides). */
    const float* w2;
    const float* scale2;
    const float* shift2;
    int32_t cin_pad2, cout_pad2;
} esm_shuffle_conv_desc;

/* Depthwise KxK conv (groups = C, no bias) + folded BN (out = act(conv * scale[c] + shift[c]); scale NULL = 1,
 * shift NULL = 0): timm's conv_dw + bn of the backbone blocks (models/ESMStereo.py:40-77).  x: [B, C, H, W]
 * (strides xb, xc, xh; innermost 1), w: [C][K][K], out: [B, C, Ho, Wo] (strides ob, oc, oh), zero padding
 * `pad`, (K, stride) in {(3, 1), (3, 2), (5, 1), (5, 2)}, act one of ESM_ACT_*. */
typedef struct {
    const float* x;
    int64_t xb, xc, xh;
    const float* w;
    const float* scale;
    const float* shift;
    float* out;
    int64_t ob, oc, oh;
    int32_t B, C, H, W, K, stride, pad, act, Ho, Wo;
} esm_dwconv_desc;

const char* esm_last_error(void);
int esm_version(void);
/* sizeof of the ABI structs, for binding checks: 0 esm_src, 1 esm_conv_desc,
 * 2 esm_smix_stage, 3 esm_smix_desc, 4 esm_shuffle_tail_desc, 5 esm_fmnet_desc, 6 esm_conf_desc,
 * 8 esm_shuffle_conv_desc, 9 esm_dwconv_desc, 10 esm_cloud_desc;
 * -1 for an unknown id. */
int esm_struct_size(int which);

int esm_gwc_volume_f32(const float* L, const float* R, const float* att, float* V, int B, int C, int H, int W,
                       int D, int G, void* stream);
/* The gwc volume and the first 3-D conv over it in one launch (ESMStereo-L / -M: build_gwc_volume,
 * models/submodule.py:151-161, then group_stem, models/ESMStereo.py:610-611 / 703-704): `stem` describes the
 * conv as esm_conv_f32 would take it over the [B, G, D, H, W] volume (Cin = G, Di x Hi x Wi = D x H x W,
 * 3x3x3 stride 1 pad 1, <= 8 outputs; its src[] is ignored and no volume is written); L / R are contiguous
 * [B, C, H, W] features with C = 2 G, G a multiple of 4.  Bit-identical to esm_gwc_volume_f32 followed by
 * esm_conv_f32 with the LDS-tiled form (ESM_HINT_TILE); ESM_HINT_ROWS(2 / 3) in stem->hint: rows per wave 2 / 4. */
int esm_gwc_stem_f32(const esm_conv_desc* stem, const float* L, const float* R, int C, int G, void* stream);
/* Whether esm_gwc_stem_f32 takes these arguments: ESM_OK, or the launch's negative status with its message.  The
 * same checks as the launch; nothing is launched, L / R are compared with NULL only and nothing is read through the
 * descriptor's pointers. */
int esm_gwc_stem_check(const esm_conv_desc* stem, const float* L, const float* R, int C, int G);
int esm_concat_volume_f32(const float* L, const float* R, float* V, int B, int C, int H, int W, int D,
                          void* stream);
/* work: unused since the single-launch kernel (normalises in LDS); may be NULL.  C <= 64. */
int esm_normcorr_volume_f32(const float* L, const float* R, float* V, float* work, int B, int C, int H, int W,
                            int D, void* stream);
int esm_disp_regression_f32(const float* cost, float* out, int B, int D, int H, int W, void* stream);
/* samples: [B, D, H, W] disparity_samples, or NULL for arange(D) (the ESMStereo call). */
int esm_topk2_regression_f32(const float* cost, const float* samples, float* out, int B, int D, int H, int W,
                             void* stream);
/* regression_topk for any k >= 1 (models/submodule.py:218-225): the reference slices the sorted
 * indices, so k > D selects all D.  Ties rank the lower index first; NaN ranks first. */
int esm_topk_regression_f32(const float* cost, const float* samples, float* out, int B, int D, int H, int W, int k,
                            void* stream);
int esm_conv_f32(const esm_conv_desc* desc, void* stream);
/* The form esm_conv_f32 takes for `desc` (an ESM_FORM_* value): the same validation and the same rules, and
 * nothing is launched or read through the descriptor's pointers.  A form forced through `hint` is reported as
 * forced (its launcher may still refuse the layer), except the two that step aside for the automatic rules:
 * WIDE when the sources do not share a row stride, and the pointwise form when the layout does not suit it.
 * Negative (ESM_ERR_ARG, message set) for a descriptor esm_conv_f32 refuses before choosing a form. */
#define ESM_FORM_GENERAL 0 /* direct / LDS-staged implicit GEMM (conv2d.hip, conv3d.hip), its rows and C1T variants */
#define ESM_FORM_STEM 1    /* conv_stem.hip, 16-block narrow-output form */
#define ESM_FORM_C1IN 2    /* conv_stem.hip, VALU single-input-channel form */
#define ESM_FORM_SMALL 3   /* conv_small.hip */
#define ESM_FORM_WIDE 4    /* conv_wide.hip */
#define ESM_FORM_WIDE3 5   /* conv_wide3.hip */
#define ESM_FORM_WIDET 6   /* conv_widet.hip */
#define ESM_FORM_TILE3 7   /* conv_tile3.hip, 3-D */
#define ESM_FORM_TILE2 8   /* conv_tile3.hip, 2-D */
#define ESM_FORM_PW 9      /* conv_pw.hip */
int esm_conv_form(const esm_conv_desc* desc);
/* Whether the VALU single-output-channel ConvTranspose form (csrc/conv_c1.h; ESM_HINT_C1T, and the automatic
 * rules' first choice within ESM_FORM_GENERAL) can run `desc`: 1 or 0; nothing is launched or read through the
 * descriptor's pointers.  0 for a source whose per-item span or strides lie beyond its 32-bit buffer offsets: the
 * automatic rules then take a 64-bit form, which esm_conv_form reports as ESM_FORM_GENERAL as well.  Negative
 * (ESM_ERR_ARG, message set) for a descriptor esm_conv_f32 refuses. */
int esm_convt_c1_ok(const esm_conv_desc* desc);
/* Which kernel a lean (ESM_FORM_SMALL) launch of `desc` runs, for tests and tools; nothing is launched or read
 * through the descriptor's pointers.  1: the kernel behind the first-load record, whose 14 dwords are written to
 * rec (layout: csrc/conv_lean_rec.h; one source, extents / strides / pads within the packed fields, BN constants
 * [scale | shift] directly behind the packed weights as engine.pack_conv lays them out) and, unpacked again, to the
 * 19 values of fields (the pointers excluded): sb sc sd sh m_ds m_b Wi Hi Di Ws Ds B Cin cout_pad pd ph pw xcd scale.
 * 0: the struct-argument kernel (a layer the record cannot describe, or ESM_HINT_SMALL_NO_RECORD). */
int esm_lean_record_pack(const esm_conv_desc* desc, uint32_t rec[14], int64_t fields[19]);
/* The first-load record of the 2-D single-output-channel ConvTranspose kernel, for tests and tools; nothing is
 * launched or read through the descriptor's pointers.  esm_c1_record_pack writes the 16 dwords of `desc` launched on
 * `grid` (x, y, z workgroups) to rec (layout: csrc/conv_c1_rec.h) and, unpacked again, the 16 values of fields: src w
 * sb sc sh Hi Wi Cin cin_pad cout_pad slab gx gy nwg m_gx m_gy; it packs the fields as given (what the form runs is
 * esm_convt_c1_ok's answer).  esm_c1_record_tile writes to xyz the tile that the workgroup dispatched as (bx, by, bz)
 * computes under `rec`: the host side of the kernel's own map.  Both return 1, or ESM_ERR_ARG for a null argument. */
int esm_c1_record_pack(const esm_conv_desc* desc, const uint32_t grid[3], uint32_t rec[16], int64_t fields[16]);
int esm_c1_record_tile(const uint32_t rec[16], uint32_t bx, uint32_t by, uint32_t bz, int32_t xyz[3]);
int esm_smix_f32(const esm_smix_desc* desc, void* stream);
int esm_fmnet_f32(const esm_fmnet_desc* desc, void* stream);
int esm_shuffle_tail_f32(const esm_shuffle_tail_desc* desc, void* stream);
int esm_shuffle_conv_f32(const esm_shuffle_conv_desc* desc, void* stream);
/* The fused launches' form queries, in the manner of esm_conv_form: each applies the argument checks and the rules
 * of the launch it is named after, launches nothing and reads nothing through the descriptors' pointers (they are
 * compared with NULL and with each other, and their alignment is read), so it needs no device.  Negative: the status
 * the launch would return, with its message.  A form one of them names is the form the launch runs for the same
 * descriptors; the one refusal a launch can still add is a shuffle head's grid of more than 65535 tiles down or
 * batch items ("grid too large"), which depends on the tile the named form then picks.
 *
 * esm_shuffle_tail_form: the kernel of esm_shuffle_tail_f32.  ROW4 / ROW8: the (nf 8, r 4) head's row form with 4 / 8
 * low-resolution rows per workgroup (flags bits 1-2 = 2 / 3; automatically 8 rows where they still give >= 128
 * workgroups); WINDOW: every other head, flags bits 1-2 = 1, and the automatic rule's smaller maps. */
#define ESM_SHUFFLE_TAIL_FORM_WINDOW 0
#define ESM_SHUFFLE_TAIL_FORM_ROW4 1
#define ESM_SHUFFLE_TAIL_FORM_ROW8 2
int esm_shuffle_tail_form(const esm_shuffle_tail_desc* desc);
/* esm_shuffle_conv_form: the kernel of esm_shuffle_conv_f32.  WINDOW: every head but (nf 8, r 4, C 16), that head
 * under st.flags bits 1-2 = 1 and on the automatic rule's smaller maps (under 128 workgroups of 8 low-resolution
 * rows).  ROW_VALU / ROW_MFMA: its row form with the refinement conv on the VALU (bits 1-2 = 2) or the matrix cores
 * (3, the pre-conv without 2, and automatically), ORed with PRE when the launch computes the pre-conv (pre_x) too.
 * CONV1 + t: the whole conv1 in the launch (w2), t = st.flags bits 3-4, its tile. */
#define ESM_SHUFFLE_CONV_FORM_WINDOW 0
#define ESM_SHUFFLE_CONV_FORM_ROW_VALU 1
#define ESM_SHUFFLE_CONV_FORM_ROW_MFMA 2
#define ESM_SHUFFLE_CONV_FORM_PRE 4
#define ESM_SHUFFLE_CONV_FORM_CONV1 8
int esm_shuffle_conv_form(const esm_shuffle_conv_desc* desc);
/* Two consecutive BasicConvs in one launch (the intermediate map stays in LDS; halo recomputed):
 * out_b = GELU(BN_b(conv_b(GELU(BN_a(conv_a(cat(a->src))))))).  a: k 1/3/5 stride 1 or k 3 stride 2,
 * 16 outputs, <= 48 input channels (64 for k 1) over 1..3 sources (4-channel multiples when several);
 * a->out is not written.  b: k 1 or 3, stride 1, 16 inputs (its src[] is ignored: the input is a's
 * output), <= 16 outputs, plain epilogue.  ESM_ERR_ARG for a pair outside that set.
 * Regression source (ESM_HINT_PAIR_REGRESS in a->hint; a: 5x5, Cin 1, one source; b: 3x3): a->src[0] is a
 * [B, D, H, W] cost volume (src[0].C = D, H x W = a's input extent) and a's input map is its disparity_regression
 * sum_d cost[d] * d (models/submodule.py:211-216, the bits of esm_disp_regression_f32), which is also
 * stored to a->out ([B, 1, H, W], strides ob / oh): the regression launch folded into the upsampler's
 * first pair (models/ESMStereo.py:735-745).  b->hint ESM_HINT_ROWS(1 / 2 / 3): tile rows 2 / 4 / 8 (8 only with
 * <= 16 input channels; of b->hint's other bits only ESM_HINT_PAIRK, below, and ESM_HINT_PAIR_NO_RECORD are read), 0 = automatic (4 rows where
 * that gives >= 256 tiles).
 * (models/ESMStereo.py:185-259: the refinement hourglasses' conv2 / conv3 pairs and the upsampler
 * stages' dm<t> / spx_<t> pairs.)
 * K-split form (conv_pairk.hip; ESM_HINT_PAIRK in b->hint, and automatically for a pair only it runs): a: 2-D or
 * 3-D k 3 stride 1 or 2 padding 1, <= 48 input channels over 1..3 sources, <= 32 outputs; b: k 3 stride 1 padding 1
 * over a's outputs (same dimensionality), <= 32 outputs; BN + GELU and a plain store on both; b->hint
 * ESM_HINT_ROWS(1 / 2 / 3): tile rows 1 / 2 / 4, 0 = automatic (the fewest that keep the grid within 256
 * workgroups).  Not with the regression source.  (models/ESMStereo.py:129-182: the 3-D aggregation hourglass's
 * conv1 / conv2 / conv3 are pairs of this shape; the package takes the form for 2-D pairs of <= 4096 output pixels, engine.pairk_auto.) */
int esm_conv_pair2_f32(const esm_conv_desc* a, const esm_conv_desc* b, void* stream);
/* The form esm_conv_pair2_f32 takes for the pair, hints included (ESM_HINT_PAIRK and ESM_HINT_ROWS in b->hint,
 * ESM_HINT_PAIR_REGRESS in a->hint): the LDS-staged or the K-split form.  A query as described above
 * esm_shuffle_tail_form; a named form is one the launch runs (its grid limits and the regressed map's cover by the
 * tiles are part of the answer).  ESM_ERR_ARG, message set, for a pair esm_conv_pair2_f32 refuses. */
#define ESM_PAIR_FORM_LDS 1
#define ESM_PAIR_FORM_KSPLIT 2
int esm_conv_pair2_form(const esm_conv_desc* a, const esm_conv_desc* b);
/* Which kernel an LDS-form launch of the pair runs, for tests and tools; nothing is launched or read through the
 * descriptors' pointers.  1: the kernel behind the staging record, whose 20 dwords are written to rec (layout:
 * csrc/conv_pair2_rec.h; sources with one channel and row stride, extents / strides / pads within the packed
 * fields, weights packed as engine.pack_weight packs them -- cin_pad = Cin rounded up to 16, cout_pad = 32, 16-byte
 * aligned -- with the BN constants [scale | shift] directly behind them as engine.pack_conv lays them out) and,
 * unpacked again, to the 24 values of fields: src0 wa wb sb0 sc sh Wi Hi Cin pa pb CoutB nsrc xcd D src1 src2 sb1 sb2
 * C0 C01 out ob oh (out ob oh alias src1 sb1 sb2; they are the stored map's with ESM_HINT_PAIR_REGRESS).
 * 0: the struct-argument kernel (a pair the record cannot describe, or ESM_HINT_PAIR_NO_RECORD in b->hint), or a pair
 * for which esm_conv_pair2_form does not answer ESM_PAIR_FORM_LDS. */
int esm_pair2_record_pack(const esm_conv_desc* a, const esm_conv_desc* b, uint32_t rec[20], int64_t fields[24]);
/* A ConvTranspose BasicConv and the 1x1 BasicConv over [its output cropped to b's extent, further sources]
 * in one launch; replaces the decoder steps of models/ESMStereo.py:163-175 (aggregation: conv3_up ->
 * cat(crop, conv2) -> agg_0[0], conv2_up -> cat(crop, conv1) -> agg_1[0]) and :221-234 (up_refinement, with
 * left_f1x / left_f2x as the third source).  out_b = GELU(BN_b(conv1x1_b(cat(crop(GELU(BN_a(convT_a(a->src)))),
 * b->src[1..])))).  a: k4 s2 p1, one source, 4 / 8 / 12 / 16 outputs, BN + GELU, plain epilogue; a->out is
 * not written (may be NULL).  b: 1x1 stride 1, b->src[0].C = a->Cout (its ptr is not read; b's input extent
 * is the crop, at most a's output extent), b->src[1..2]: 4-channel multiples, at most 48 channels together;
 * <= 16 outputs, BN + GELU, plain epilogue.  a->hint picks the transposed conv's form (ESM_HINT_TILE: LDS-tiled,
 * ESM_HINT_ROWS(1 / 2) rows per wave; ESM_HINT_SMALL: lean), 0 = automatic.  ESM_ERR_ARG outside that set. */
int esm_convt_1x1_f32(const esm_conv_desc* a, const esm_conv_desc* b, void* stream);
/* The form esm_convt_1x1_f32 takes for the pair under a->hint: the lean or the LDS-tiled form of the transposed
 * conv.  A query as described above esm_shuffle_tail_form; a named form is one the launch runs (what the form's
 * launcher cannot run -- the transposed conv's layout, two cout tiles in 2-D, its grid limits -- is part of the
 * answer).  ESM_ERR_ARG, message set, for a pair esm_convt_1x1_f32 refuses. */
#define ESM_UP1_FORM_LEAN 1
#define ESM_UP1_FORM_TILED 2
int esm_convt_1x1_form(const esm_conv_desc* a, const esm_conv_desc* b);
/* Confidence-head stages (models/ESMStereo_confidence.py), fp32 NCHW, contiguous:
 *   ESM_CONF_COST_FEATURES  x[0] = cost [B,D,H,W] (D >= 7) -> out [B,7,H,W]: the 7 largest of
 *                           softmax(-100 * cost / sqrt(sum_d cost^2 + 1e-6)) over D, descending (:647-654)
 *   ESM_CONF_ATTEND         x[0..2] = cost_x, disp_x, imag_x [B,C,H,W], x[3] = logits [B,3,H,W] ->
 *                           out [B,3C,H,W] = cat(x_k * softmax_k(logits)) (:679-689)
 *   ESM_CONF_ENLARGE        x[0] = feat [B,C,H,W], x[1] = scale [B,1,H,W] -> out [B,9C,H,W]: the 3x
 *                           enlarged grid_sample(feat, grid(scale), bilinear, align_corners, zeros) of
 *                           :691-714, stored space-to-depth (channel c*9 + 3i + j = sample (3y+i, 3x+j)),
 *                           so embed_conv2 (k3 s3) runs as a 1x1 conv over 9C channels
 *   ESM_CONF_COMBINE        x[0] = logits [B,9,4H,4W], x[1] = init [B,1,H,W] -> out [B,1,4H,4W] =
 *                           sum_k softmax_k(logits) * unfold3x3(init)[k] at (Y/4, X/4) (:538-543)
 *   ESM_CONF_SIGMOID        x[0] [B*C*H*W] -> out, torch.sigmoid (:744) */
#define ESM_CONF_COST_FEATURES 1
#define ESM_CONF_ATTEND 2
#define ESM_CONF_ENLARGE 3
#define ESM_CONF_COMBINE 4
#define ESM_CONF_SIGMOID 5
typedef struct {
    int32_t op;
    int32_t B, C, D, H, W;
    const float* x[4];
    float* out;
} esm_conf_desc;
int esm_conf_f32(const esm_conf_desc* desc, void* stream);
/* The backbone's depthwise conv + BN + activation (esm_dwconv_desc; replaces MIOpen's grouped conv + BatchNorm +
 * activation of timm's blocks, backbone side of models/ESMStereo.py:640-697). */
int esm_dwconv_f32(const esm_dwconv_desc* desc, void* stream);

/* img: [B, H, W, 3] uint8 RGB (PIL order); out: [B, 3, Hp, Wp] fp32.  The image lands at rows
 * [top, top+H), columns [left, left+W); pad_normalized = 1 fills the rest with normalised zeros
 * (test_kitti.py: top = Hp-H, left = Wp-W), 0 with 0.0 (kitti_dataset.py: top = Hp-H, left = 0). */
int esm_preprocess_u8(const uint8_t* img, float* out, int B, int H, int W, int Hp, int Wp, int top, int left,
                      int pad_normalized, void* stream);
/* disp: [B, Hp, Wp] fp32; out: [B, h, w] uint16 = round_half_even(disp[b, top+y, left+x] * 256). */
int esm_disp_to_u16(const float* disp, uint16_t* out, int B, int Hp, int Wp, int top, int left, int h, int w,
                    void* stream);

/* The ROS node's post-processing (kitti_publisher/src/kitti_publisher_cuda_node.cpp:385-403) on the
 * device: disp [B, Hp, Wp] fp32 -> window (top, left, h, w) -> 5x5 median (cv::medianBlur, replicate
 * border inside the window) -> 0 outside (0, max_disp) -> out [B, h, w] uint16 =
 * saturate_cast<ushort>(rint(d * 256)); `filtered` (may be NULL) receives the masked median [B, h, w]. */
int esm_node_filter_u16(const float* disp, uint16_t* out, float* filtered, int B, int Hp, int Wp, int top, int left,
                        int h, int w, float max_disp, void* stream);

/* ---- scoring a disparity against ground truth (utils/metrics.py, utils/visualization.py) ---- */
#define ESM_METRICS_MAX_THRES 4
#define ESM_METRICS_PARTIAL_BYTES 48   /* workspace bytes per workgroup of the first pass */
#define ESM_METRICS_RECORD_DOUBLES 12  /* n_mask, n_gt_pos, sum_abs_err, reserved, n_abs[4], n_both[4] */
#define ESM_METRICS_VALUES 10          /* epe, thres[4], d1[4], skipped (per image) / images kept (batch) */
/* Bytes of `workspace` esm_disp_metrics_f32 needs for a [B, H, W] batch: ESM_METRICS_PARTIAL_BYTES per partial
 * record, the same number of records for every image.  ESM_ERR_ARG (negative) for a non-positive size or
 * H * W >= 2^31. */
long long esm_disp_metrics_workspace(int B, int H, int W);
/* EPE_metric, D1_metric, D1_metric_thres and Thres_metric of utils/metrics.py:42-74 with the per-image skip rule
 * and batch mean of compute_metric_for_each_image (:17-39), for nthres <= 4 thresholds, in one pass and two
 * launches, with no host sync.  est, gt: fp32 [B, H, W]; mask: one byte per pixel (torch.bool), NULL = every
 * pixel.  Each is addressed by its own batch and row stride in elements (W contiguous), so a crop
 * pred[:, hi-h:, wi-w:] (test_kitti.py:114) is read in place.  use_range != 0 ANDs the mask with
 * gt > lo && gt < hi: the `(disp_gt < maxdisp) & (disp_gt > 0)` of train_kitti.py:221 / test_kitti.py:120
 * without a mask tensor.  `thres` is a HOST array of nthres values; rel is D1's relative bound (0.05f).
 * With E = |gt - est| (fp32) over the masked pixels of one image:
 *   records [B, 12] fp64: n_mask, n_gt_pos (gt > 0 over the whole image), sum of E (fp64, fixed order),
 *           0, n_abs[k] = #(E > thres[k]), n_both[k] = #(E > thres[k] && E / |gt| > rel); counts are exact;
 *   values  [B, 10] fp32: epe = float(sum / n_mask), thres[k] = float(n_abs[k]) / float(n_mask),
 *           d1[k] = float(n_both[k]) / float(n_mask) (entries k >= nthres are 0), skipped = 1.0 when
 *           (n_mask / HW) / (n_gt_pos / HW) < 0.1f in fp32 (utils/metrics.py:26; NaN keeps the image);
 *   batch   [10] fp32: the first nine values averaged over the kept images in image order (fp32; 0 when
 *           every image is skipped, utils/metrics.py:31-37), then the number of kept images.
 * Two runs on the same input give the same bits.  ESM_ERR_ARG: null est / gt / workspace / outputs,
 * nthres outside 0..4, a negative stride, B > 65535, H * W >= 2^31. */
int esm_disp_metrics_f32(const float* est, int64_t est_sb, int64_t est_sh, const float* gt, int64_t gt_sb,
                         int64_t gt_sh, const uint8_t* mask, int64_t mask_sb, int64_t mask_sh, int B, int H, int W,
                         float lo, float hi, int use_range, const float* thres, int nthres, float rel,
                         void* workspace, double* records, float* values, float* batch, void* stream);
/* The KITTI error image `vis` of utils/visualization.py:20-37 (test_kitti.py:134): out [B, 3, H, W] fp32,
 * contiguous.  mask = gt > 0; err = min(E / abs_thres, (E / gt) / rel_thres) with IEEE divisions; the colour of
 * the table row with lo <= err < hi (utils/visualization.py:4-18), 0 outside the mask or when no row holds err;
 * then the legend, rows < 10, columns [20 i, 20 (i + 1)) = colour i, clipped to the image.  Bit-exact. */
int esm_disp_error_map_f32(const float* est, int64_t est_sb, int64_t est_sh, const float* gt, int64_t gt_sb,
                           int64_t gt_sh, float* out, int B, int H, int W, float abs_thres, float rel_thres,
                           void* stream);

/* ---- rendering a disparity: colour-mapped 8-bit frames and depth (save_vid.py, the ROS node, latest.py) ---- */
#define ESM_COLORIZE_SCALE 0 /* idx from the x256 16-bit value times alpha (save_vid.py:119-122 and its twins) */
#define ESM_COLORIZE_RANGE 1 /* idx from each image's own min / max (kitti_publisher_cuda_node.cpp:81-85) */
#define ESM_COLORIZE_DEPTH 2 /* idx from the clipped depth (latest.py:54-64) */
/* Bytes of `workspace` esm_disp_colorize_u8 needs in RANGE mode for a [B, H, W] batch (8 bytes per workgroup of the
 * range pass and per image).  ESM_ERR_ARG (negative) for a non-positive size or H * W >= 2^31. */
long long esm_disp_colorize_workspace(int B, int H, int W);
/* disp: fp32 [B, H, W] addressed by a batch and a row stride in elements (W contiguous, element alignment only), so
 * a crop of a padded map is read where it lies.  lut: uint8 [256, 3] on the device, in the output's channel order.
 * out: uint8 [B, Hout, W, 3] contiguous, pixel = lut[idx].  top_frames (may be NULL): uint8 [B, H, W, 3]
 * contiguous; with it Hout = 2 H, rows [0, H) are a byte copy of the frame and rows [H, 2 H) the colour image
 * (np.concatenate((left_img, disp_np), 0) / cv::vconcat); without it Hout = H.  idx by mode:
 *   SCALE  u = the value esm_disp_to_u16 writes; idx = saturate_u8(rint(float(u) * alpha)), round half to even
 *          (cv2.convertScaleAbs(np.round(d * 256).astype(np.uint16), alpha = 0.01): u >= 25550 gives 255).
 *   RANGE  disp is the masked median `filtered` of esm_node_filter_u16 (invalid pixels are 0): valid = m > 0,
 *          u = valid ? min(rint(m * 256), 65535) : 0; per image mn, mx = the integer min, max of u over the valid
 *          pixels; a = float(-255.0 / (mx - mn)), b = float(255.0 * mx / (mx - mn)), each computed in fp64 on the
 *          device and rounded once; idx = saturate_u8(rint(float(u) * a + b)), a separate multiply and add, for
 *          every pixel, valid or not (minMaxLoc over the mask, then convertTo(CV_8UC1, a, b) of the whole map).
 *          DEFINED HERE: the reference divides by zero when no pixel is valid or mx == mn; that image is idx = 0
 *          everywhere.  The range never leaves the device; `workspace` holds the partial ranges.
 *   DEPTH  depth = num / d (IEEE fp32; num = float(baseline * focal), rounded once by the caller), clipped to
 *          [0, max_depth] with NaN kept (np.clip); n = clip(depth / max_depth, 0, 1); u8 = (uint8)(n * 255),
 *          truncated, DEFINED HERE as 0 for NaN; idx = 255 - u8 (latest.py:56-63).  The substitution of 1e-6 for
 *          d <= 0 (latest.py:55) is the caller's step.
 * alpha is read in SCALE mode only, num and max_depth in DEPTH mode only.  One launch (SCALE, DEPTH) or two to
 * three (RANGE), no host sync.  ESM_ERR_ARG: null disp / lut / out, a non-positive size, a negative stride, an
 * unknown mode, B > 65535, H * W >= 2^31, RANGE without a workspace. */
int esm_disp_colorize_u8(const float* disp, int64_t disp_sb, int64_t disp_sh, int B, int H, int W, int mode,
                         float alpha, float num, float max_depth, const uint8_t* lut, const uint8_t* top_frames,
                         uint8_t* out, void* workspace, void* stream);
/* The clipped depth map itself: out [B, H, W] fp32 contiguous = clip(num / d, 0, max_depth) as in DEPTH mode
 * above (latest.py:56-57), bit-exact with the numpy lines.  disp is addressed as in esm_disp_colorize_u8. */
int esm_disp_to_depth_f32(const float* disp, int64_t disp_sb, int64_t disp_sh, float* out, int B, int H, int W,
                          float num, float max_depth, void* stream);

/* ---- the confidence-gated node and the depth-image node (kitti_publisher_conf, virtual_kitti_publisher) ---- */
/* kitti_publisher_conf/src/kitti_publisher_conf_cuda_node.cpp:555-576.  disp, conf: fp32 [B, Hp, Wp], both read
 * through the window (top, left, h, w).  m = the 5x5 median of disp with the border replicated inside the window,
 * as esm_node_filter_u16 takes it (the confidence is not filtered);
 *   valid = (m > 0) && (m < max_disp) && ((double)conf >= threshold)
 * in fp64, because the node compares a float matrix against the double slider / 100.0 (:490,571): float32(0.29) <
 * 0.29, so an fp32 comparison would flip such pixels.  A NaN confidence is invalid.  Where not valid, m = 0.
 * out [B, h, w] uint16 = saturate_cast<ushort>(rint(m * 256)); `filtered` (may be NULL) receives m; `valid` (may be
 * NULL) one byte per pixel, 1 or 0 (a torch.bool view; the `mask` of esm_disp_metrics_f32).  conf == NULL turns the
 * gate off: on NaN-free input the three outputs are then those of esm_node_filter_u16, bit for bit.  One launch; the
 * median is selected from an LDS tile, exactly.  ESM_ERR_ARG: null disp / out, a non-positive size, a window outside
 * the map. */
int esm_node_filter_conf_u16(const float* disp, const float* conf, uint16_t* out, float* filtered, uint8_t* valid,
                             int B, int Hp, int Wp, int top, int left, int h, int w, float max_disp,
                             double threshold, void* stream);
/* The frame of visualize_and_record_disparity (kitti_publisher_conf_cuda_node.cpp:183-257) without what the node
 * draws on it (circle, putText).  filtered: fp32 [B, h, w] contiguous, the masked median of the entry above; conf:
 * fp32 [B, Hp, Wp] read through the window (top, left, h, w), may be NULL (Hp, Wp, top, left are then ignored);
 * gt16: uint16 [B, h, w], the KITTI 16-bit ground truth, may be NULL; left_img: uint8 [B, h, w, 3]; lut: uint8
 * [256, 3]; workspace: esm_disp_colorize_workspace(B, h, w) bytes.  out: uint8 [B, 2h, 2w, 3] contiguous, the panels
 * of vconcat / vconcat / hconcat (:250-257):
 *   top-left      a byte copy of left_img;
 *   bottom-left   lut[idx], idx exactly as ESM_COLORIZE_RANGE defines it for `filtered` (its DEFINED-HERE empty
 *                 range included);
 *   top-right     the node's own `vis` (:94-151; not utils/visualization.py's): gt = float(gt16) * (1.f / 256.f), 0
 *                 where filtered is not > 0 (:211-213); mask = gt > 0; E = |gt - filtered|; err = min(E, E / gt),
 *                 IEEE fp32; the colour of the row with lo <= err < hi of gen_error_colormap (:69-92), whose fp32
 *                 bounds are 0, 1/16, 1/8, 1/4, 1/2, 1, 2, 4, 8, 16, +inf; bytes (col4, col3, col2) (the table is RGB,
 *                 then COLOR_RGB2BGR, :220), each saturate_u8(rint((c / 255.f) * 255.f)) = c; black outside the mask,
 *                 when no row holds err, and when gt16 is NULL.  No legend;
 *   bottom-right  saturate_u8(rint(conf * 256.f)) in all three channels (:204-205); DEFINED HERE: NaN gives 0; black
 *                 when conf is NULL.
 * gt_f32 (may be NULL): fp32 [B, h, w], the masked ground truth above (0 everywhere when gt16 is NULL): with
 * est = filtered and use_range on (0, 192) esm_disp_metrics_f32 gives computeEPE (:55-67) as records[2] / records[0].
 * Two launches (three above a million pixels), no host sync.  ESM_ERR_ARG: null filtered / left_img / lut / out /
 * workspace, a non-positive size, B > 65535, h * w >= 2^31, with conf a window outside its map. */
int esm_node_panels_u8(const float* filtered, const float* conf, int Hp, int Wp, int top, int left,
                       const uint16_t* gt16, const uint8_t* left_img, const uint8_t* lut, uint8_t* out, float* gt_f32,
                       void* workspace, int B, int h, int w, void* stream);
/* virtual_kitti_publisher/src/virtual_kitti_publisher_cuda_node.cpp:55-77 (depthToDisparity) and :146-147
 * (cv::resize(..., INTER_LINEAR)) in one launch.  depth16: uint16 [B, Hs, Ws]; out: fp32 [B, H, W].  The source value
 * is s = (z <= 0) ? 0 : num / z with z = float(d16) * depth_scale and num = float(focal) * float(baseline), rounded
 * once by the caller.  The resize restates OpenCV's float INTER_LINEAR rule: scale = (double)Ws / W;
 * fx = (float)((x + 0.5) * scale - 0.5); sx = floor(fx); fx -= sx (fp32); sx < 0: sx = 0, fx = 0; sx >= Ws - 1:
 * sx = Ws - 1, fx = 0; the neighbour is min(sx + 1, Ws - 1); the same in y; horizontally first,
 * r = s[x0] * (1 - fx) + s[x1] * fx on each of the two rows, then r0 * (1 - fy) + r1 * fy, each operation rounded in
 * fp32.  With Hs == H and Ws == W the result is s itself, bit for bit.  Parity with OpenCV's own bytes is UNPINNED.
 * ESM_ERR_ARG: a null pointer, a non-positive size, Hs * Ws or H * W >= 2^31. */
int esm_depth16_to_disp_f32(const uint16_t* depth16, float* out, int B, int Hs, int Ws, int H, int W, float num,
                            float depth_scale, void* stream);

/* ---- the resizing nodes' front end (virtual_kitti_publisher, kitti_publisher_ess): any camera, one size ---- */
/* cv::resize(src, dst, Size(W, H), 0, 0, INTER_LINEAR) of an 8-bit image.  src: uint8 [B, Hs, Ws, C], dst: uint8
 * [B, H, W, C], both interleaved and contiguous, C = 1 or 3.  THE RESIZE RULE is a definition of this library: it
 * restates OpenCV's 8-bit INTER_LINEAR (11-bit fixed-point coefficients, int32 accumulation) as its source reads, and
 * parity with OpenCV's own bytes is UNPINNED (cv2 is importable nowhere this is built or tested).
 *   Taps.  Along each axis, for output index i of n_dst from n_src samples, (i0, i1, f) are those of
 *     esm_depth16_to_disp_f32 above: t = (float)((i + 0.5) * ((double)n_src / n_dst) - 0.5); i0 = floor(t);
 *     f = t - i0 (fp32); i0 < 0: i0 = 0, f = 0; i0 >= n_src - 1: i0 = n_src - 1, f = 0; i1 = min(i0 + 1, n_src - 1).
 *   Coefficients.  a0 = rint((1.f - f) * 2048.f), a1 = rint(f * 2048.f): fp32 products rounded half to even into an
 *     int (horizontally a0, a1 at x0, x1; vertically b0, b1 at y0, y1).
 *   Horizontal pass, per channel, in int32, on rows y0 and y1:  D = S[x0] * a0 + S[x1] * a1.
 *   Vertical pass:  v = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2, stored as a byte.
 * With Hs == H and Ws == W dst is src, byte for byte (a0 = b0 = 2048).  One launch, no LDS, no host sync.
 * ESM_ERR_ARG, each decided before any HIP call: a null src / dst, a non-positive size, C outside {1, 3}, B > 65535,
 * Hs * Ws * C or H * W * C >= 2^31. */
int esm_resize_u8(const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int H, int W, int C, void* stream);
/* preprocess_image of the resizing nodes in one launch: the resize above, then the network input.  img: uint8
 * [B, Hs, Ws, 3]; out: fp32 [B, 3, H, W], the resized byte u of channel c as ((float)u / 255 - mean[c]) / stdv[c],
 * each operation rounded in fp32 (esm_preprocess_u8's arithmetic).  mean, stdv: HOST arrays of 3, applied to channel
 * c as stored (the nodes feed OpenCV's BGR and never swap it); the ESS node passes 0 and 1.  resized (may be NULL):
 * uint8 [B, H, W, 3], the bytes esm_resize_u8 gives for the same image, from the same launch: the left image's call
 * yields the network input and the picture's top panel together (:186-188).  With Hs == H, Ws == W and the ImageNet
 * constants out is esm_preprocess_u8's on the same bytes without padding.  ESM_ERR_ARG as esm_resize_u8 with C = 3,
 * and a null img / out / mean / stdv. */
int esm_preprocess_resize_u8(const uint8_t* img, float* out, uint8_t* resized, int B, int Hs, int Ws, int H, int W,
                             const float* mean, const float* stdv, void* stream);

/* ---- PNG encoding on the device (save_disp.py:83-88, test_kitti.py:127-131: the writer behind the 16-bit map) ---- */
/* Per image, one complete zlib stream (RFC 1950) holding one deflate block (RFC 1951), Huffman-only:
 *   78 01;  BFINAL = 1, BTYPE = 2, HLIT = 0 (257 codes: literals and end-of-block), HDIST = 0 (one distance code of
 *   length 1, never used), HCLEN = 15, the code-length alphabet fixed as "symbols 0-15: 4 bits, 16-18: 0 bits" sent in
 *   the RFC's permuted order, so each of the 258 lengths is one 4-bit code and the block header is always 1106 bits;
 *   the image's own canonical code (3.2.2; at most 15 bits, complete), bit-reversed into the LSB-first stream, over
 *   the filtered scanlines, then end-of-block;  padding to a byte;  the big-endian Adler-32 of the filtered scanlines.
 * Filtered scanlines: per row one filter-type byte, then the row; 16-bit samples big-endian, colour as R, G, B.  The
 * filter is one per call: 0 None, 1 Sub (bpp 2 for maps, 3 for frames), 2 Up.  The caller wraps the stream in the
 * PNG signature, IHDR, one IDAT with its CRC-32 and IEND (esmstereo_amd/io.py); there is no LZ77 matching.
 *
 * The host-only calls below touch no device. */
/* Bytes of raw (filtered) data one workgroup encodes. */
int esm_png_chunk_bytes(void);
/* An upper bound of the stream of raw_bytes filtered bytes (rows * (1 + bytes per row)), a multiple of 16:
 * 2 + ceil((1106 + 9 (raw_bytes + 1)) / 8) + 4 rounded up.  The flat complete code (255 symbols of 8 bits, 2 of 9)
 * never costs more than 9 bits a symbol and the encoder never does worse than it.  ESM_ERR_ARG: raw_bytes <= 0 or
 * >= 2^28. */
long long esm_png_stream_bound(long long raw_bytes);
/* Bytes of the device workspace of a batch of B images of `rows` rows of `row_bytes` sample bytes (2 w for a map, 3 w
 * for a frame; the filter byte is added here).  ESM_ERR_ARG: a non-positive size, rows * (1 + row_bytes) >= 2^28. */
long long esm_png_workspace_bytes(int B, int rows, int row_bytes);
/* Code lengths for the counts hist[0 .. 256] (literals, then end-of-block, which is counted once when its count is
 * 0): at most 15 bits, a zero count gets length 0, and the non-zero lengths form a complete code.  Optimal (Huffman)
 * whenever an optimal code fits 15 bits; otherwise length-limited and never costlier than the flat code over the
 * symbols present.  The function the device runs per image (csrc/deflate_lengths.h).  With nothing but end-of-block
 * literal 0 gets the second code.  ESM_ERR_ARG: a null pointer, counts summing to 2^32 or more. */
int esm_deflate_code_lengths(const uint32_t hist[257], uint8_t len[257]);
/* The 1106 bits of the block header for those lengths, LSB-first from out[0]; the 6 unused bits of out[138] are 0;
 * *nbits (may be NULL) receives 1106.  ESM_ERR_ARG: a null len / out, a length above 15. */
int esm_deflate_header(const uint8_t len[257], uint8_t out[139], int* nbits);
/* The device calls.  src: uint16 [B, h, w] / uint8 [B, h, w, 3] (bgr != 0: stored B, G, R) / for the disparity entry
 * fp32 [B, Hp, Wp], of which the window (top, left, h, w) is encoded as esm_disp_to_u16 would round it, without the
 * uint16 map ever being stored.  All contiguous.  work: esm_png_workspace_bytes bytes, 4-byte aligned, contents
 * arbitrary.  out: B slots of slot_stride bytes (a multiple of 4, >= esm_png_stream_bound; 4-byte aligned), contents
 * arbitrary: image b's stream is out[b * slot_stride .. + lengths[b]); up to 3 bytes behind it may be zeroed and
 * nothing else of the slot is written.  lengths: DEVICE int32 [B].  Three stream-ordered launches (filter and count;
 * table and scan; emit), no host synchronisation; the bytes are identical from run to run.
 * ESM_ERR_ARG, each decided before any pointer is touched and before any HIP call: an unknown filter, a non-positive
 * size, B > 65535, h * (1 + 2 w) (1 + 3 w for frames) >= 2^28, a slot smaller than the bound or not a multiple of 4,
 * a null or misaligned pointer, a window outside the map. */
int esm_png_encode_u16(const uint16_t* src, int B, int h, int w, void* work, uint8_t* out, long long slot_stride,
                       int32_t* lengths, int filter, void* stream);
int esm_png_encode_rgb8(const uint8_t* src, int B, int h, int w, int bgr, void* work, uint8_t* out,
                        long long slot_stride, int32_t* lengths, int filter, void* stream);
int esm_png_encode_disp_f32(const float* disp, int B, int Hp, int Wp, int top, int left, int h, int w, void* work,
                            uint8_t* out, long long slot_stride, int32_t* lengths, int filter, void* stream);

/* ---- JPEG encoding on the device (the nodes' MJPG video writer: kitti_publisher_cuda_node.cpp:122-132,
 * kitti_publisher_conf_cuda_node.cpp:265-275, virtual_kitti_publisher_cuda_node.cpp:218-228,
 * kitti_publisher_ess_cuda_node.cpp:227-237: cv::VideoWriter 'MJPG', video_writer.write(combined)) ---- */
/* A baseline JFIF encoder, defined by the rules below and not by bit-parity with libjpeg or OpenCV (UNPINNED: cv2 is
 * importable nowhere this library is built); any baseline decoder reads its files.  tests/jpeg_ref.py restates it.
 * Input: uint8 [B, H, W, 3] contiguous, stored R, G, B or (bgr != 0) B, G, R.  1 <= H, W <= 65535, B <= 65535,
 *   3 H W < 2^31.  quality 1..100; subsampling 420 or 444; restart_mcus (Ri) 1..16.
 * Padding: to a multiple of the MCU (16 x 16 for 420, 8 x 8 for 444) by replicating the last column and row of pixels.
 * Colour: full-range BT.601 in int32 with arithmetic shifts:
 *   Y  = ( 19595 R + 38470 G +  7471 B +   32768) >> 16
 *   Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16        (8421375 = 128 * 65536 + 32767)
 *   Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16        all three stay in 0..255.
 * Chroma (420): (a + b + c + d + 2) >> 2 over each 2 x 2 of the padded Cb / Cr.
 * Forward DCT on s = v - 128 with M[k][n] = round(8192 * 1/2 C(k) cos((2n + 1) k pi / 16)), C(0) = 1/sqrt 2, else 1
 *   (row 0: 2896 x 8; row 1: 4017 3406 2276 799 -799 -2276 -3406 -4017):
 *   rows first     t[y][u]  = (sum_n M[u][n] s[y][n] +  512) >> 10
 *   then columns   c8[v][u] = (sum_y M[v][y] t[y][u] + 4096) >> 13      (8 x the coefficient; every sum fits int32)
 * Quantisation: q = sgn(c8) ((|c8| + 4 Q) / (8 Q)), integer division; AC values are clamped to +-1023 (a guard that
 *   no input reaches).  Q: Annex K.1 (luminance) / K.2 (chrominance) scaled as libjpeg does: s = quality < 50 ?
 *   5000 / quality : 200 - 2 quality, Q = clamp((base s + 50) / 100, 1, 255).
 * Entropy coding: baseline, zigzag order, the Annex K.3 Huffman tables.  DC: the difference from the previous block
 *   of the same component; AC: (run, size) with ZRL for runs above 15, EOB unless coefficient 63 is non-zero; a
 *   negative value v is coded as v + 2^size - 1; bits MSB-first; a 0x00 follows every 0xFF data byte.
 * MCUs in raster order; a 420 MCU is Y00 Y01 Y10 Y11 Cb Cr.
 * Restarts: before MCU m (m > 0, m mod Ri == 0) the current byte is padded with 1-bits, FF D0+((m / Ri - 1) & 7) is
 *   emitted and the three DC predictors return to 0.  After the last MCU: padding with 1-bits, then FF D9.
 * Header (esm_jpeg_header, 629 bytes): FF D8; FF E0 00 10 'JFIF\0' 01 01 00 00 01 00 01 00 00; FF DB 00 43 00 + the
 *   luminance table in zigzag order, FF DB 00 43 01 + the chrominance table; FF C0 00 11 08 HH HH WW WW 03 | 01 sf 00
 *   | 02 11 01 | 03 11 01 (sf 0x22 for 420, 0x11 for 444); four FF C4 segments in class/id order 00, 10, 01, 11;
 *   FF DD 00 04 + Ri; FF DA 00 0C 03 01 00 02 11 03 11 00 3F 00.
 *
 * The four host-only calls touch no device. */
/* The 64 entries of table `which` (0 luminance, 1 chrominance) at `quality`, natural (row-major) order.
 * ESM_ERR_ARG: null out64, quality outside 1..100, which not 0 / 1. */
int esm_jpeg_quant_table(int quality, int which, uint8_t out64[64]);
/* Writes the header above into buf[0 .. cap) and returns its length (629).  ESM_ERR_ARG: null buf, cap below 629,
 * sizes or parameters outside the limits. */
int esm_jpeg_header(uint8_t* buf, int cap, int w, int h, int quality, int subsampling, int restart_mcus);
/* The most bytes the scan of an h x w image can take, restart markers and EOI included: per restart interval of n
 * MCUs of 6 (420) or 3 (444) blocks 2 ceil(n blocks * 1658 / 8) + 2.  A block is at most 20 + 63 * 26 bits (a 9-bit
 * DC code and 11 value bits; 63 times a 16-bit AC code and 10 value bits), and byte stuffing at most doubles the
 * bytes.  ESM_ERR_ARG: sizes or parameters outside the limits. */
long long esm_jpeg_stream_bound(int h, int w, int subsampling, int restart_mcus);
/* Bytes of the device workspace of a batch of B such images: 12 per restart interval.  ESM_ERR_ARG as above and for
 * B outside 1..65535. */
long long esm_jpeg_workspace_bytes(int B, int h, int w, int subsampling, int restart_mcus);
/* The device call (video_writer.write(combined), the lines above).  work: esm_jpeg_workspace_bytes bytes, 8-byte
 * aligned, contents arbitrary.  out: B slots of slot_bytes bytes, contents arbitrary: image b's scan (every interval,
 * its RSTn markers, EOI) is out[b * slot_bytes .. + lengths[b]); esm_jpeg_header's bytes go in front of it.  Nothing
 * else of the slot is written.  lengths: DEVICE int32 [B], the scan's length with EOI.  When a scan does not fit
 * slot_bytes, lengths[b] = -needed (INT32_MIN when needed >= 2^31), the slot holds a truncated scan, nothing outside
 * it is written, and the status is still ESM_OK: encode again into slots of `needed` (esm_jpeg_stream_bound always
 * suffices).  Three stream-ordered launches (encode and count per restart interval; scan the lengths into offsets;
 * encode again and place), no host synchronisation, no allocation; each output byte has exactly one writer, so the
 * bytes are identical from run to run.
 * ESM_ERR_ARG, each decided before any pointer is touched and before any HIP call: a null pointer, sizes or
 * parameters outside the limits above, slot_bytes < 2, a misaligned work. */
int esm_jpeg_encode_rgb8(const uint8_t* src, int B, int h, int w, int bgr, int quality, int subsampling,
                         int restart_mcus, void* work, uint8_t* out, long long slot_bytes, int32_t* lengths,
                         void* stream);

/* ---- point clouds: the 3-D points of a disparity map, compacted and coloured, as a plan op ---- */
/* The rectified pinhole camera of the reference node (fx, baseline: kitti_publisher_cuda_node.cpp:60-78,277-278) and
 * the depth of latest.py:54-58, carried on to XYZ(RGB).  The op has no entry point of its own: it is added to a plan
 * with esm_plan_add_cloud and runs through esm_plan_run / esm_plan_graph_build / esm_plan_graph_launch.
 *   disp, disp_sb, disp_sh  fp32 [B, H, W] addressed by a batch and a row stride in elements (W contiguous, element
 *                           alignment only), exactly as esm_disp_colorize_u8 addresses it: a crop of a padded map is
 *                           read where it lies.
 *   color                   uint8 [B, H, W, 3] contiguous, or NULL; bgr != 0: stored B, G, R, else R, G, B.
 *   valid                   uint8 [B, H, W] contiguous, or NULL: the `valid` of esm_node_filter_conf_u16, non-zero
 *                           means usable.
 *   step                    >= 1: only pixels with x % step == 0 && y % step == 0 are candidates.
 *   num, fx, fy, cx, cy, z_min, z_max   fp32; num = float(fx * baseline), rounded once by the caller, as in
 *                           esm_disp_to_depth_f32.
 *   packing                 the order of a record's colour bytes (below).
 *   out, slot_points        the records of image b start at record b * slot_points of `out` (16-byte aligned);
 *                           slot_points >= esm_cloud_max_points(H, W, step).
 *   counts                  int32 [B] on the device.
 *   work                    esm_cloud_workspace_bytes(B, H, W, step) bytes, 4-byte aligned, contents arbitrary.
 * Per candidate pixel (x, y) with d = disp[b, y, x], every operation rounded in fp32, none contracted:
 *   Z = num / d
 *   X = ((float)x - cx) * Z / fx        (left to right)
 *   Y = ((float)y - cy) * Z / fy
 *   keep = d > 0 && Z >= z_min && Z <= z_max && (valid == NULL || valid[b, y, x] != 0)
 * A NaN fails every comparison, so it is dropped.  Results in the fp32 denormal range are UNPINNED.
 * The kept points of image b are written densely from record 0 of its slot, in raster order of (y, x), and
 * counts[b] is their number.  Nothing behind record counts[b] of a slot is written, and the bytes are the same from
 * run to run.  A record is 12 bytes (X, Y, Z) without `color`, and with it 16: X, Y, Z and four bytes,
 *   ESM_CLOUD_PACK_PLY  R, G, B, 255    (the properties of a PLY vertex: x y z red green blue alpha)
 *   ESM_CLOUD_PACK_PCL  B, G, R, 0      (the `rgb` field of a ROS PointCloud2 read as uint32 0x00RRGGBB).
 * Three stream-ordered launches for the whole batch (count per tile of esm_cloud_tile_points() candidates, scan per
 * image, emit per tile), no host sync, no workgroup waiting on another.
 * ESM_ERR_ARG, each decided before any pointer is followed and before any HIP call: a null disp / out / counts /
 * work; a misaligned pointer; a non-positive size or step; a negative stride; B > 65535; H * W >= 2^31; slot_points
 * below the bound; B * slot_points * record bytes >= 2^40; an unknown packing; fx or fy not finite or zero;
 * z_min > z_max or either NaN. */
#define ESM_CLOUD_PACK_PLY 0
#define ESM_CLOUD_PACK_PCL 1
typedef struct {
    const float* disp;
    int64_t disp_sb, disp_sh;
    const uint8_t* color;
    const uint8_t* valid;
    void* out;
    int64_t slot_points;
    int32_t* counts;
    void* work;
    int32_t B, H, W, step;
    int32_t bgr, packing;
    float num, fx, fy, cx, cy, z_min, z_max;
    int32_t reserved;
} esm_cloud_desc;
/* Candidates per workgroup of the count and emit launches (host only). */
int esm_cloud_tile_points(void);
/* The most points one image can give: ceil(H / step) * ceil(W / step) (host only).  ESM_ERR_ARG (negative) for a
 * non-positive size or step or H * W >= 2^31. */
long long esm_cloud_max_points(int H, int W, int step);
/* Bytes of `work` for a [B, H, W] batch: 4 per tile (host only).  ESM_ERR_ARG as above, and for B > 65535. */
long long esm_cloud_workspace_bytes(int B, int H, int W, int step);
/* The record size of an acceptable descriptor, 12 or 16, or ESM_ERR_ARG as listed above; touches no device. */
int esm_cloud_check(const esm_cloud_desc* desc);

/* ---- native launch plan (the hot path as one replayable unit) ---- */
typedef struct esm_plan esm_plan;
esm_plan* esm_plan_create(void);
void esm_plan_destroy(esm_plan* plan);
int esm_plan_add_conv(esm_plan* plan, const esm_conv_desc* desc);
int esm_plan_add_smix(esm_plan* plan, const esm_smix_desc* desc);
int esm_plan_add_fmnet(esm_plan* plan, const esm_fmnet_desc* desc);
int esm_plan_add_shuffle_tail(esm_plan* plan, const esm_shuffle_tail_desc* desc);
int esm_plan_add_shuffle_conv(esm_plan* plan, const esm_shuffle_conv_desc* desc);
int esm_plan_add_conv_pair2(esm_plan* plan, const esm_conv_desc* a, const esm_conv_desc* b);
int esm_plan_add_convt_1x1(esm_plan* plan, const esm_conv_desc* a, const esm_conv_desc* b);
int esm_plan_add_gwc(esm_plan* plan, const float* L, const float* R, const float* att, float* V, int B, int C,
                     int H, int W, int D, int G);
int esm_plan_add_gwc_stem(esm_plan* plan, const esm_conv_desc* stem, const float* L, const float* R, int C, int G);
int esm_plan_add_concat(esm_plan* plan, const float* L, const float* R, float* V, int B, int C, int H, int W,
                        int D);
int esm_plan_add_normcorr(esm_plan* plan, const float* L, const float* R, float* V, float* work, int B, int C,
                          int H, int W, int D);
/* kind 0 = disparity_regression, 1 = regression_topk k=2, 2 + k = regression_topk with that k */
int esm_plan_add_regression(esm_plan* plan, int kind, const float* cost, float* out, int B, int D, int H, int W);
int esm_plan_add_conf(esm_plan* plan, const esm_conf_desc* desc);
/* The point cloud op (esm_cloud_desc above): refused with esm_cloud_check's errors, the plan unchanged. */
int esm_plan_add_cloud(esm_plan* plan, const esm_cloud_desc* desc);
int esm_plan_num_ops(const esm_plan* plan);
/* 0 = unknown, 1 = conv, 2 = smix, 3 = gwc, 4 = concat, 5 = normcorr, 6 = regression,
 * 7 = shuffle_tail, 9 = fmnet, 10 = conf, 12 = shuffle_conv, 13 = conv_pair2, 14 = gwc_stem, 15 = convt_1x1,
 * 16 = cloud (8 and 11 were retired fused forms) */
int esm_plan_op_kind(const esm_plan* plan, int index);
/* Replace the tile hint of conv op `index` (see esm_conv_desc.hint); returns the previous hint
 * (>= 0) or an error.  ESM_HINT_XCD_SLAB (tile order) is kept as the op was added, and is not part of the
 * returned value.  Drops a built graph (rebuild with esm_plan_graph_build). */
int esm_plan_set_conv_hint(esm_plan* plan, int index, int hint);
/* Diagnostics: launch op `index` `repeat` times per replay (0..8; 0 drops it, so the step time
 * minus the dropped step time is the op's marginal cost in the chain, gaps included).  Returns the
 * previous count; drops a built graph.  Results of a plan with a dropped op are not meaningful. */
int esm_plan_set_repeat(esm_plan* plan, int index, int repeat);
int esm_plan_run(esm_plan* plan, void* stream);
/* Launch op `index` alone, `reps` times back to back on `stream` (timing one kernel of the
 * path with a single hipEvent pair around the batch; the op's buffers are the plan's own). */
int esm_plan_run_op(esm_plan* plan, int index, int reps, void* stream);
/* Capture the launch list into a hipGraph (instantiated once; replays are cheap).  graph_launch
 * builds the graph first when there is none (never built, or dropped by a hint / repeat / probe change
 * or a rebind that changed an op's kernel). */
int esm_plan_graph_build(esm_plan* plan, void* stream);
int esm_plan_graph_launch(esm_plan* plan, void* stream);
/* Zero-copy input binding: every pointer of every op that lies in [old_base[k], old_base[k] + bytes[k])
 * moves to the same offset in new_base[k], k < n (the caller's tensors are read where they lie, the
 * reference forward's behaviour, models/ESMStereo.py:700-745).  With a built graph, the nodes of the
 * ops that changed are updated in place (after the previous replay has finished); when an op's
 * kernel choice changes with its pointers, the graph is dropped and rebuilt by the next launch.
 * Returns the number of pointer fields moved, or an error: ESM_ERR_ARG when two old ranges overlap
 * (which range a pointer belongs to would be ambiguous; bind aliased inputs through copies).  When
 * waiting for the previous replay fails, the ops are already moved and the graph is dropped (rebuilt
 * from the moved ops by the next launch). */
int esm_plan_rebind(esm_plan* plan, int n, const void* const* old_base, const uint64_t* bytes,
                    const void* const* new_base);
/* 1 while the last graph replay of the plan may still be running on the device (a rebind would then
 * wait for it), 0 when it has finished or the plan was never launched as a graph; < 0 on error. */
int esm_plan_busy(esm_plan* plan);
/* Probe: record a hipEvent pair around op `index` on every run/replay (ring of `ring`
 * pairs, ring <= 4096).  esm_plan_probe_read returns the elapsed ms of the completed
 * runs since the last read (caller synchronises first); returns the count written. */
int esm_plan_set_probe(esm_plan* plan, int index, int ring);
int esm_plan_probe_read(esm_plan* plan, float* ms, int max);

/* ---- diagnostics: choosing what a kernel inherits in LDS (tests/lds_poison.py) ---- */
/* LDS is not cleared between workgroups or launches: a kernel that reads a cell it never wrote reads what the
 * previous kernel on that CU left there.  esm_lds_fill_u32 writes `pattern` into all 163,840 B of LDS of every CU
 * of the current device (workgroups that each declare the whole 160 KiB, esm_lds_probe_workgroups() of them: 8 per
 * CU), so that the next launch on `stream` inherits it. */
int esm_lds_fill_u32(uint32_t pattern, void* stream);
/* The same geometry, writing nothing to LDS: workgroup wg stores the number of the 40,960 words of its 160 KiB that
 * differ from `pattern` to out[2 wg] and the identity of its CU (XCC id << 16 | the CU, SH and SE fields of HW_ID)
 * to out[2 wg + 1].  out: a DEVICE array of 2 * n_workgroups words, n_workgroups >= esm_lds_probe_workgroups().
 * ESM_ERR_ARG, before any launch: null out, n_workgroups too small. */
int esm_lds_probe_u32(uint32_t pattern, uint32_t* out, int n_workgroups, void* stream);
/* The grid of both launches on the current device (8 x its CU count); negative without a device. */
int esm_lds_probe_workgroups(void);

#ifdef __cplusplus
}
#endif

#endif /* ESMSTEREO_AMD_H */
