// The fixed-size front end of the reference's two resizing ROS nodes, virtual_kitti_publisher and kitti_publisher_ess:
// every camera frame is resized to the network size, not padded.
//
//  esm_resize_u8  cv::resize(..., INTER_LINEAR) of an 8-bit interleaved image (the picture's squeeze,
//    virtual_kitti_publisher_cuda_node.cpp:211-213, and the left image at the network size, :186-188).
//  esm_preprocess_resize_u8  preprocess_image (:232-266; kitti_publisher_ess_cuda_node.cpp:241-275): the same resize,
//    then /255, mean and std into planar fp32 (esm_preprocess_u8's arithmetic), in one launch; the resized bytes
//    themselves are a second, optional output of that launch.
//
// OpenCV's 8-bit INTER_LINEAR rule (11-bit coefficients, int32 accumulation) is restated in the header; parity with
// OpenCV's own bytes is UNPINNED.
//
// Shape.  A gather of four taps per output and memory- and launch-bound: no LDS.  A thread owns four consecutive
// output pixels of one row, so the interleaved bytes leave as whole dwords (4 bytes for C = 1, render_range.h's
// 12-byte store_group for C = 3) and the three planar fp32 rows as one 16-byte store each where the address allows.
// The vertical taps are computed once per thread, the horizontal ones per pixel; the source bytes are byte loads that
// L1 / L2 serve (neighbouring lanes read neighbouring bytes of the same two rows).
#include "render_range.h"

// the coordinate is an fp64 expression rounded to fp32, the fraction an fp32 difference, each rounded once
#pragma clang fp contract(off)

namespace esm {
namespace {

using rdr::kThreads;

constexpr int kPix = 4;        // output pixels per thread
constexpr int kCoefBits = 11;  // INTER_RESIZE_COEF_BITS
constexpr float kCoefScale = static_cast<float>(1 << kCoefBits);

struct Tap {
    int i0, i1, c0, c1;
};

// OpenCV's INTER_LINEAR taps of output index i along an axis of n source samples, and their 11-bit coefficients
__device__ __forceinline__ Tap linear_tap(int i, double scale, int n) {
    float f = static_cast<float>((i + 0.5) * scale - 0.5);
    int s = static_cast<int>(floorf(f));
    f -= static_cast<float>(s);
    if (s < 0) s = 0, f = 0.f;
    if (s >= n - 1) s = n - 1, f = 0.f;
    Tap t;
    t.i0 = s;
    t.i1 = min(s + 1, n - 1);
    t.c0 = static_cast<int>(rintf((1.f - f) * kCoefScale));
    t.c1 = static_cast<int>(rintf(f * kCoefScale));
    return t;
}

struct ResizeArgs {
    const uint8_t* src;  // [B, Hs, Ws, C]
    uint8_t* dst;        // [B, H, W, C]; may be NULL with PRE
    float* out;          // PRE: [B, 3, H, W]
    int Hs, Ws, H, W;
    int groups_per_row;
    double scale_y, scale_x;
    float mean[3], stdv[3];
};

// n <= 4 floats to o: one 16-byte store where the address allows
__device__ __forceinline__ void store_row4(float* __restrict__ o, const float (&v)[kPix], int n) {
    if (n == kPix && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (i < n) o[i] = v[i];
    }
}

// n <= 4 bytes, the little-endian contents of r, to o
__device__ __forceinline__ void store_bytes4(uint8_t* __restrict__ o, uint32_t r, int n) {
    if (n == kPix && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(o) = r;
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (i < n) o[i] = static_cast<uint8_t>(r >> (8 * i));
    }
}

template <int C, bool PRE>
__global__ void __launch_bounds__(kThreads) resize_kernel(const ResizeArgs k) {
    static_assert(C == 1 || C == 3, "interleaved grey or colour");
    static_assert(!PRE || C == 3, "the network input has three channels");
    const int b = blockIdx.y;
    const uint32_t g = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;  // group of four pixels in a row
    const uint32_t y = g / static_cast<uint32_t>(k.groups_per_row);
    if (y >= static_cast<uint32_t>(k.H)) return;
    const int x0 = static_cast<int>(g - y * k.groups_per_row) * kPix;
    const int n = min(kPix, k.W - x0);
    const Tap ty = linear_tap(static_cast<int>(y), k.scale_y, k.Hs);
    const uint8_t* img = k.src + static_cast<long long>(b) * k.Hs * k.Ws * C;  // Hs * Ws * C < 2^31: int below
    const uint8_t* row0 = img + ty.i0 * k.Ws * C;
    const uint8_t* row1 = img + ty.i1 * k.Ws * C;
    int v[kPix][C];
#pragma unroll
    for (int i = 0; i < kPix; ++i) {
        // a pixel past the row's end takes the last pixel's taps: inside the source, never stored
        const Tap tx = linear_tap(min(x0 + i, k.W - 1), k.scale_x, k.Ws);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            // horizontal pass on the two rows, then the vertical one: int32, OpenCV's shifts
            const int d0 = row0[tx.i0 * C + c] * tx.c0 + row0[tx.i1 * C + c] * tx.c1;
            const int d1 = row1[tx.i0 * C + c] * tx.c0 + row1[tx.i1 * C + c] * tx.c1;
            v[i][c] = (((ty.c0 * (d0 >> 4)) >> 16) + ((ty.c1 * (d1 >> 4)) >> 16) + 2) >> 2;
        }
    }
    const long long pix = (static_cast<long long>(b) * k.H + y) * k.W + x0;
    if (k.dst) {
        uint8_t* o = k.dst + pix * C;
        if constexpr (C == 1) {
            store_bytes4(o, v[0][0] | (v[1][0] << 8) | (v[2][0] << 16) | (static_cast<uint32_t>(v[3][0]) << 24), n);
        } else {
            uint32_t p[kPix], r[3];
#pragma unroll
            for (int i = 0; i < kPix; ++i) p[i] = v[i][0] | (v[i][1] << 8) | (v[i][2] << 16);
            rdr::pack_group(p, r);
            rdr::store_group(o, r, 3 * n);
        }
    }
    if constexpr (PRE) {
        const long long plane = static_cast<long long>(k.H) * k.W;
        float* o = k.out + (static_cast<long long>(b) * 3 * k.H + y) * k.W + x0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float f[kPix];
#pragma unroll
            for (int i = 0; i < kPix; ++i) f[i] = (static_cast<float>(v[i][c]) / 255.0f - k.mean[c]) / k.stdv[c];
            store_row4(o + c * plane, f, n);
        }
    }
}

// what both entry points refuse, before any HIP call
int check_sizes(const char* what, int B, int Hs, int Ws, int H, int W, int C) {
    const std::string w(what);
    if (B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return arg_error(w + ": non-positive size");
    if (C != 1 && C != 3) return arg_error(w + ": C must be 1 or 3");
    if (B > 65535) return arg_error(w + ": batch above 65535");
    if (static_cast<long long>(Hs) * Ws * C >= (1LL << 31) || static_cast<long long>(H) * W * C >= (1LL << 31))
        return arg_error(w + ": Hs * Ws * C and H * W * C must be below 2^31");
    return ESM_OK;
}

template <int C, bool PRE>
int launch(ResizeArgs& k, int B, hipStream_t s, const char* what) {
    k.groups_per_row = (k.W + kPix - 1) / kPix;
    k.scale_y = static_cast<double>(k.Hs) / k.H;
    k.scale_x = static_cast<double>(k.Ws) / k.W;
    const long long groups = static_cast<long long>(k.H) * k.groups_per_row;
    hipLaunchKernelGGL((resize_kernel<C, PRE>), dim3(ceil_div(groups, kThreads), B), dim3(kThreads), 0, s, k);
    return check_launch(what);
}

}  // namespace

int launch_resize_u8(const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int H, int W, int C, hipStream_t s) {
    if (!src || !dst) return arg_error("resize_u8: null pointer");
    if (int rc = check_sizes("resize_u8", B, Hs, Ws, H, W, C)) return rc;
    ResizeArgs k = {};
    k.src = src, k.dst = dst, k.Hs = Hs, k.Ws = Ws, k.H = H, k.W = W;
    return C == 1 ? launch<1, false>(k, B, s, "resize_u8") : launch<3, false>(k, B, s, "resize_u8");
}

int launch_preprocess_resize_u8(const uint8_t* img, float* out, uint8_t* resized, int B, int Hs, int Ws, int H, int W,
                                const float* mean, const float* stdv, hipStream_t s) {
    if (!img || !out || !mean || !stdv) return arg_error("preprocess_resize_u8: null pointer");
    if (int rc = check_sizes("preprocess_resize_u8", B, Hs, Ws, H, W, 3)) return rc;
    ResizeArgs k = {};
    k.src = img, k.dst = resized, k.out = out, k.Hs = Hs, k.Ws = Ws, k.H = H, k.W = W;
    for (int c = 0; c < 3; ++c) k.mean[c] = mean[c], k.stdv[c] = stdv[c];
    return launch<3, true>(k, B, s, "preprocess_resize_u8");
}

}  // namespace esm

extern "C" {

int esm_resize_u8(const uint8_t* src, uint8_t* dst, int B, int Hs, int Ws, int H, int W, int C, void* stream) {
    return esm::launch_resize_u8(src, dst, B, Hs, Ws, H, W, C, esm::as_stream(stream));
}

int esm_preprocess_resize_u8(const uint8_t* img, float* out, uint8_t* resized, int B, int Hs, int Ws, int H, int W,
                             const float* mean, const float* stdv, void* stream) {
    return esm::launch_preprocess_resize_u8(img, out, resized, B, Hs, Ws, H, W, mean, stdv, esm::as_stream(stream));
}

}  // extern "C"
