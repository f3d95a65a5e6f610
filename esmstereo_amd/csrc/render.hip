// Rendering a disparity on the device: the 8-bit colour-mapped frame every reference script ends in, and the depth map.
//
//  esm_disp_colorize_u8   fp32 disparity [B, H, W] -> idx in 0..255 -> lut[idx] -> uint8 [B, Hout, W, 3], optionally
//    stacked under an 8-bit frame (np.concatenate((left_img, disp_np), 0), cv::vconcat).  Three definitions of idx:
//      SCALE  save_vid.py:118-125, save_disp.py:87-97, test_mid.py:118-121, test_eth3d.py:102-105:
//             cv2.applyColorMap(cv2.convertScaleAbs(np.round(d * 256).astype(np.uint16), alpha=0.01), JET)
//             u = disp_u16_value(d) (common.h, the value esm_disp_to_u16 writes);
//             idx = saturate_u8(rint(float(u) * alpha))
//      RANGE  kitti_publisher_cuda_node.cpp:81-86: minMaxLoc over the valid mask, then
//             convertTo(CV_8UC1, -255 / (max - min), 255 * max / (max - min)) of the 16-bit map, MAGMA.
//             u = m > 0 ? min(rint(m * 256), 65535) : 0 (esm_node_filter_u16's formula on its own `filtered` map);
//             mn, mx over the valid pixels of one image; a, b in fp64, each rounded once to fp32;
//             idx = saturate_u8(rint(float(u) * a + b)), a separate multiply and add, for every pixel.
//             DEFINED HERE: no valid pixel, or mx == mn (the reference divides by zero): idx = 0 everywhere.
//      DEPTH  latest.py:56-63: depth = clip(num / d, 0, max_depth), n = clip(depth / max_depth, 0, 1),
//             idx = 255 - (uint8)(n * 255), fp32 throughout, NaN kept by the clips.  DEFINED HERE: NaN -> u8 0.
//    The arithmetic in front of the table restates OpenCV's documented semantics (saturate_cast = round half to even,
//    then clamp); parity against OpenCV's own output is UNPINNED (cv2 is importable nowhere this runs).  The table
//    is an argument: a caller with cv2 passes cv2.applyColorMap(np.arange(256, dtype=np.uint8), code).
//  esm_disp_to_depth_f32  the clipped fp32 depth map of latest.py:56-57, bit-exact with the numpy lines.
//
// Shape.  An HBM-bound stream: 4 B read and 3 B written per pixel (6 B more moved with the stack).  An image's pixels
// are taken flat, four to a group, two groups per thread, 2048 pixels per workgroup: a group is one 16-byte load when
// it lies inside a row (element alignment only: a crop's rows start anywhere) and per-pixel loads across a row's end,
// and its 12 output bytes are consecutive whatever W is, because the colour image of one frame is contiguous.  They
// leave as three dwords when the address is 4-byte aligned; otherwise (3 W (b Hout + H) is not a multiple of 4) as
// 1-3 leading bytes, two aligned dwords funnel-shifted out of the three, and the trailing bytes.  The table is
// staged in LDS once per workgroup as 256 packed dwords; lanes read it at data-dependent addresses, so equal
// indices broadcast and distinct ones on one bank serialise.
// RANGE: range_partial_kernel writes one (min, max) per workgroup, the render pass folds an image's partials itself
// (up to kFoldMax of them, one per thread or two; above that range_final_kernel folds them first), and one thread
// forms a and b: two launches, three for an image above a million pixels, no host sync.  Integer min and max: any
// order gives the same bits.
#include "render_range.h"

// every operation rounded once, as numpy / OpenCV round it
#pragma clang fp contract(off)

namespace esm {
namespace {

using namespace rdr;  // the RANGE definition and the group stores, shared with node_conf.hip

constexpr int kGroups = 2;                         // groups of four pixels per thread
constexpr int kTilePix = kThreads * kGroups * 4;   // 2048 pixels per workgroup
constexpr int kFoldMax = 512;                      // partial ranges per image the render pass folds itself

struct RenderArgs {
    const float* disp;
    long long sb, sh;
    int H, W, tiles, mode;
    float alpha, num, max_depth;
    const uint8_t* lut;
    const uint8_t* top;
    uint8_t* out;
    RangeRef range;  // RANGE: where the range pass left the partials
};

__device__ __forceinline__ int index_scale(float d, float alpha) {
    return sat_u8(rintf(static_cast<float>(disp_u16_value(d)) * alpha));
}

// np.clip: a NaN stays, and so does -0.0 against a bound of 0
__device__ __forceinline__ float clipf(float x, float lo, float hi) {
    x = x < lo ? lo : x;
    return x > hi ? hi : x;
}

__device__ __forceinline__ float depth_clipped(float d, float num, float max_depth) {
    return clipf(num / d, 0.0f, max_depth);
}

__device__ __forceinline__ int index_depth(float d, float num, float max_depth) {
    const float n = clipf(depth_clipped(d, num, max_depth) / max_depth, 0.0f, 1.0f);
    const float v = n * 255.0f;
    return 255 - (v != v ? 0 : static_cast<int>(v));
}

// The n <= 4 pixels from flat index p0 of one image.  Inside a row: one 16-byte load.  Only element alignment is
// assumed, which gfx950's global loads need and no more.  Across a row's end (and for W < 4): a load per pixel.
__device__ __forceinline__ void load_group(const float* __restrict__ img, long long sh, int W, uint32_t p0, int n,
                                           float (&v)[4]) {
    const uint32_t y = p0 / static_cast<uint32_t>(W);
    const uint32_t x = p0 - y * static_cast<uint32_t>(W);
    if (n == 4 && x + 4 <= static_cast<uint32_t>(W)) {
        __builtin_memcpy(v, img + y * sh + x, 16);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = 0.0f;
            if (i < n) {
                const uint32_t yi = (p0 + i) / static_cast<uint32_t>(W);
                v[i] = img[yi * sh + ((p0 + i) - yi * static_cast<uint32_t>(W))];
            }
        }
    }
}

__global__ void __launch_bounds__(kThreads) range_partial_kernel(const float* __restrict__ disp, long long sb,
                                                                 long long sh, int H, int W, int tiles,
                                                                 Range* __restrict__ ws) {
    const int b = blockIdx.y;
    const float* img = disp + b * sb;
    const uint32_t npix = static_cast<uint32_t>(H) * static_cast<uint32_t>(W);
    Range r = {0xFFFFFFFFu, 0u};
    float v[kGroups][4];
    int n[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const uint32_t p0 = blockIdx.x * static_cast<uint32_t>(kTilePix) + (j * kThreads + threadIdx.x) * 4u;
        n[j] = p0 < npix ? static_cast<int>(min(4u, npix - p0)) : 0;
        load_group(img, sh, W, p0, n[j], v[j]);
    }
#pragma unroll
    for (int j = 0; j < kGroups; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n[j] && v[j][i] > 0.0f) {
                const uint32_t u = range_u(v[j][i]);
                r = merge(r, Range{u, u});
            }
    __shared__ Range part[kWaves];
    r = block_range(r, part);
    if (threadIdx.x == 0) ws[static_cast<long long>(b) * tiles + blockIdx.x] = r;
}

// one workgroup per image: its `tiles` partials -> out[b]
__global__ void __launch_bounds__(kThreads) range_final_kernel(const Range* __restrict__ ws, int tiles,
                                                               Range* __restrict__ out) {
    const Range* p = ws + static_cast<long long>(blockIdx.x) * tiles;
    Range r = {0xFFFFFFFFu, 0u};
    for (int t = threadIdx.x; t < tiles; t += kThreads) r = merge(r, p[t]);
    __shared__ Range part[kWaves];
    r = block_range(r, part);
    if (threadIdx.x == 0) out[blockIdx.x] = r;
}

__global__ void __launch_bounds__(kThreads) render_kernel(const RenderArgs k) {
    const int b = blockIdx.y;
    const float* img = k.disp + b * k.sb;
    const uint32_t npix = static_cast<uint32_t>(k.H) * static_cast<uint32_t>(k.W);
    // the loads go out first; the table and the range arrive under them
    float v[kGroups][4];
    int n[kGroups];
    uint32_t p[kGroups];
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        p[j] = blockIdx.x * static_cast<uint32_t>(kTilePix) + (j * kThreads + threadIdx.x) * 4u;
        n[j] = p[j] < npix ? static_cast<int>(min(4u, npix - p[j])) : 0;
        load_group(img, k.sh, k.W, p[j], n[j], v[j]);
    }
    __shared__ uint32_t tab[256];
    __shared__ Range part[kWaves];
    __shared__ float coef[3];  // RANGE: a, b, and whether the image has a range at all
    {
        const uint8_t* e = k.lut + 3 * threadIdx.x;
        tab[threadIdx.x] = e[0] | (e[1] << 8) | (e[2] << 16);
    }
    if (k.mode == ESM_COLORIZE_RANGE) {
        range_coefficients(k.range, b, part, coef);
    }
    __syncthreads();
    const bool ranged = k.mode == ESM_COLORIZE_RANGE && coef[2] != 0.0f;
    const float ca = ranged ? coef[0] : 0.0f, cb = ranged ? coef[1] : 0.0f;
    const long long frame = 3LL * npix;  // bytes of one colour image
    uint8_t* dst = k.out + static_cast<long long>(b) * (k.top ? 2 : 1) * frame;
    if (k.top) {
        const uint8_t* src = k.top + static_cast<long long>(b) * frame;
#pragma unroll
        for (int j = 0; j < kGroups; ++j) {
            if (n[j] == 0) continue;
            const uint8_t* s = src + 3LL * p[j];
            uint32_t r[3] = {0, 0, 0};
            if (n[j] == 4 && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
                const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
                r[0] = s4[0], r[1] = s4[1], r[2] = s4[2];
            } else {
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    if (i < 3 * n[j]) r[i / 4] |= static_cast<uint32_t>(s[i]) << (8 * (i % 4));
            }
            store_group(dst + 3LL * p[j], r, 3 * n[j]);
        }
        dst += frame;
    }
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        if (n[j] == 0) continue;
        uint32_t c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float d = v[j][i];
            int idx;
            if (k.mode == ESM_COLORIZE_SCALE)
                idx = index_scale(d, k.alpha);
            else if (k.mode == ESM_COLORIZE_DEPTH)
                idx = index_depth(d, k.num, k.max_depth);
            else
                idx = ranged ? sat_u8(rintf(static_cast<float>(range_u(d)) * ca + cb)) : 0;
            c[i] = tab[idx];
        }
        const uint32_t r[3] = {c[0] | (c[1] << 24), (c[1] >> 8) | (c[2] << 16), (c[2] >> 16) | (c[3] << 8)};
        store_group(dst + 3LL * p[j], r, 3 * n[j]);
    }
}

__global__ void __launch_bounds__(kThreads) depth_kernel(const float* __restrict__ disp, long long sb, long long sh,
                                                         float* __restrict__ out, int H, int W, float num,
                                                         float max_depth) {
    const int b = blockIdx.y;
    const float* img = disp + b * sb;
    const uint32_t npix = static_cast<uint32_t>(H) * static_cast<uint32_t>(W);
    float* o = out + static_cast<long long>(b) * npix;
#pragma unroll
    for (int j = 0; j < kGroups; ++j) {
        const uint32_t p0 = blockIdx.x * static_cast<uint32_t>(kTilePix) + (j * kThreads + threadIdx.x) * 4u;
        if (p0 >= npix) continue;
        const int n = static_cast<int>(min(4u, npix - p0));
        float v[4];
        load_group(img, sh, W, p0, n, v);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = depth_clipped(v[i], num, max_depth);
        if (n == 4) {
            __builtin_memcpy(o + p0, v, 16);  // element alignment: an image starts at b H W floats
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < n) o[p0 + i] = v[i];
        }
    }
}

bool size_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && static_cast<long long>(H) * W < (1LL << 31);
}

long long tiles_of(int H, int W) { return (static_cast<long long>(H) * W + kTilePix - 1) / kTilePix; }

}  // namespace

long long colorize_workspace(int B, int H, int W) {
    if (!size_ok(B, H, W)) return arg_error("disp_colorize_workspace: sizes must be positive and H * W below 2^31");
    return static_cast<long long>(B) * (tiles_of(H, W) + 1) * static_cast<long long>(sizeof(Range));
}

int launch_range_pass(const float* disp, long long sb, long long sh, int B, int H, int W, void* workspace,
                      hipStream_t s, RangeRef* where) {
    const int tiles = static_cast<int>(tiles_of(H, W));
    Range* ws = static_cast<Range*>(workspace);
    hipLaunchKernelGGL(range_partial_kernel, dim3(tiles, B), dim3(kThreads), 0, s, disp, sb, sh, H, W, tiles, ws);
    if (int rc = check_launch("disp_colorize (range)")) return rc;
    *where = {ws, tiles, tiles};
    if (tiles > kFoldMax) {
        Range* folded = ws + static_cast<long long>(B) * tiles;
        hipLaunchKernelGGL(range_final_kernel, dim3(B), dim3(kThreads), 0, s, ws, tiles, folded);
        if (int rc = check_launch("disp_colorize (range fold)")) return rc;
        *where = {folded, 1, 1};
    }
    return ESM_OK;
}

int launch_colorize(const float* disp, long long sb, long long sh, int B, int H, int W, int mode, float alpha,
                    float num, float max_depth, const uint8_t* lut, const uint8_t* top, uint8_t* out, void* workspace,
                    hipStream_t s) {
    if (!size_ok(B, H, W)) return arg_error("disp_colorize: sizes must be positive and H * W below 2^31");
    if (!disp || !lut || !out) return arg_error("disp_colorize: null pointer");
    if (sb < 0 || sh < 0) return arg_error("disp_colorize: negative stride");
    if (mode != ESM_COLORIZE_SCALE && mode != ESM_COLORIZE_RANGE && mode != ESM_COLORIZE_DEPTH)
        return arg_error("disp_colorize: unknown mode");
    if (mode == ESM_COLORIZE_RANGE && !workspace) return arg_error("disp_colorize: RANGE mode needs a workspace");
    if (B > 65535) return arg_error("disp_colorize: batch above 65535");
    RenderArgs k = {};
    k.disp = disp, k.sb = sb, k.sh = sh;
    k.H = H, k.W = W, k.tiles = static_cast<int>(tiles_of(H, W)), k.mode = mode;
    k.alpha = alpha, k.num = num, k.max_depth = max_depth;
    k.lut = lut, k.top = top, k.out = out;
    const dim3 grid(k.tiles, B);
    if (mode == ESM_COLORIZE_RANGE)
        if (int rc = launch_range_pass(disp, sb, sh, B, H, W, workspace, s, &k.range)) return rc;
    hipLaunchKernelGGL(render_kernel, grid, dim3(kThreads), 0, s, k);
    return check_launch("disp_colorize");
}

int launch_depth(const float* disp, long long sb, long long sh, float* out, int B, int H, int W, float num,
                 float max_depth, hipStream_t s) {
    if (!size_ok(B, H, W)) return arg_error("disp_to_depth: sizes must be positive and H * W below 2^31");
    if (!disp || !out) return arg_error("disp_to_depth: null pointer");
    if (sb < 0 || sh < 0) return arg_error("disp_to_depth: negative stride");
    if (B > 65535) return arg_error("disp_to_depth: batch above 65535");
    hipLaunchKernelGGL(depth_kernel, dim3(static_cast<unsigned>(tiles_of(H, W)), B), dim3(kThreads), 0, s, disp, sb, sh,
                       out, H, W, num, max_depth);
    return check_launch("disp_to_depth");
}

}  // namespace esm

extern "C" {

long long esm_disp_colorize_workspace(int B, int H, int W) { return esm::colorize_workspace(B, H, W); }

int esm_disp_colorize_u8(const float* disp, int64_t disp_sb, int64_t disp_sh, int B, int H, int W, int mode,
                         float alpha, float num, float max_depth, const uint8_t* lut, const uint8_t* top_frames,
                         uint8_t* out, void* workspace, void* stream) {
    return esm::launch_colorize(disp, disp_sb, disp_sh, B, H, W, mode, alpha, num, max_depth, lut, top_frames, out,
                                workspace, esm::as_stream(stream));
}

int esm_disp_to_depth_f32(const float* disp, int64_t disp_sb, int64_t disp_sh, float* out, int B, int H, int W,
                          float num, float max_depth, void* stream) {
    return esm::launch_depth(disp, disp_sb, disp_sh, out, B, H, W, num, max_depth, esm::as_stream(stream));
}

}  // extern "C"
