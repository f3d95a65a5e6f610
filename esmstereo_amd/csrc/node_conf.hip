// The per-frame device work of the reference's two other ROS nodes, kitti_publisher_conf (the confidence-gated node)
// and virtual_kitti_publisher (ground truth from a 16-bit depth image), beside esm_node_filter_u16 (io.hip) and
// esm_disp_colorize_u8 (render.hip), which cover the plain node.
//
//  esm_node_filter_conf_u16  kitti_publisher_conf_cuda_node.cpp:555-576: crop disparity and confidence to the image,
//    cv::medianBlur 5x5 of the disparity (BORDER_REPLICATE inside the crop), valid = (m > 0) & (m < max_disp) &
//    (conf >= threshold) with the threshold a double (:490), the rest set to 0, convertTo(CV_16UC1, 256.0).
//    conf == NULL: no gate, esm_node_filter_u16's result.
//    Shape.  A workgroup owns a 64 x 8 tile of the window: its 68 x 12 values (the tile and a 2-pixel halo) are staged
//    in LDS once, the replicate clamp applied to the SOURCE coordinate while staging, so a staged index is always
//    inside the window and the selection reads LDS with no clamps: 1.6 global loads per pixel instead of 25.  A thread
//    takes two vertically adjacent pixels (6 x 5 LDS reads at lane-consecutive addresses: conflict-free) and selects
//    each median with a min/max exchange network that stops at the 13th element: of 14 values neither the smallest
//    nor the largest can be the median of the 25, so both leave and the next value enters, down to a median of
//    three; 132 exchanges instead of the 300 of io.hip's full sort.  Selection only, no arithmetic: exact.
//  esm_node_panels_u8  the frame of visualize_and_record_disparity (:183-257) without what it draws on it: left
//    image | error map over colour-mapped disparity | confidence (vconcat, vconcat, hconcat, :250-257), and the fp32
//    ground truth the node scores against (:211-213).  After the range pass (render.hip's, shared through
//    render_range.h) one pass over the pixels: a thread owns four consecutive pixels of a row in all four panels, 12
//    bytes each, stored as dwords where the address allows (store_group).
//  esm_depth16_to_disp_f32  virtual_kitti_publisher_cuda_node.cpp:55-77,146-147: depthToDisparity, then
//    cv::resize(..., INTER_LINEAR) to the network size, fused: one thread per output pixel converts its four source
//    samples.  OpenCV's float INTER_LINEAR rule is restated in the header; parity with OpenCV's own bytes is UNPINNED.
#include "render_range.h"

// every operation rounded once, as OpenCV rounds it
#pragma clang fp contract(off)

namespace esm {
namespace {

using namespace rdr;

constexpr int kTileW = 64, kTileH = 8;             // pixels of the window per workgroup: 64 lanes x (4 waves x 2 rows)
constexpr int kHalo = 2;                           // 5x5
constexpr int kLdsW = kTileW + 2 * kHalo, kLdsH = kTileH + 2 * kHalo;
static_assert(kThreads == kTileW * kTileH / 2, "two pixels per thread");

__device__ __forceinline__ void cx(float& a, float& b) {
    const float lo = fminf(a, b);
    b = fmaxf(a, b);
    a = lo;
}

// the smallest of v[0..K) to v[0] and the largest to v[K-1]; the other K - 2 values stay in between
template <int K>
__device__ __forceinline__ void min_max_out(float (&v)[14]) {
#pragma unroll
    for (int i = 0; i < K / 2; ++i) cx(v[i], v[K - 1 - i]);
#pragma unroll
    for (int i = 1; i < (K + 1) / 2; ++i) cx(v[0], v[i]);
#pragma unroll
    for (int i = K / 2; i < K - 1; ++i) cx(v[i], v[K - 1]);
}

// Median of the 25 values c[r0 .. r0 + 5)[0 .. 5).  Among any 14 of them the smallest has 13 values at or above it
// and the largest 13 at or below it, so neither is needed to find the 13th of the 25: drop both, take the next.
__device__ __forceinline__ float median25(const float (&c)[6][5], int r0) {
    float v[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) v[i] = c[r0 + i / 5][i % 5];
    static_for<0, 11>([&](auto I) {
        constexpr int K = 14 - I.value;
        min_max_out<K>(v);
        v[0] = c[r0 + (14 + I.value) / 5][(14 + I.value) % 5];  // v[K - 1] is left out from here on
    });
    return fmaxf(fminf(v[0], v[1]), fminf(fmaxf(v[0], v[1]), v[2]));
}

__global__ void __launch_bounds__(kThreads) node_filter_conf_kernel(
    const float* __restrict__ disp, const float* __restrict__ conf, uint16_t* __restrict__ out,
    float* __restrict__ filtered, uint8_t* __restrict__ valid, int Hp, int Wp, int top, int left, int h, int w,
    int tiles_x, int tiles_y, float max_disp, double threshold) {
    __shared__ float tile[kLdsH][kLdsW];
    uint32_t t = blockIdx.x;
    const int bx = static_cast<int>(t % tiles_x);
    t /= tiles_x;
    const int by = static_cast<int>(t % tiles_y);
    const long long b = t / tiles_y;
    const int x0 = bx * kTileW, y0 = by * kTileH;
    const long long win = (b * Hp + top) * Wp + left;  // the window's first element
    const float* d = disp + win;
    for (int i = threadIdx.x; i < kLdsH * kLdsW; i += kThreads) {
        const int ly = i / kLdsW, lx = i - ly * kLdsW;
        const int yy = min(max(y0 + ly - kHalo, 0), h - 1);  // BORDER_REPLICATE inside the cropped window
        const int xx = min(max(x0 + lx - kHalo, 0), w - 1);
        tile[ly][lx] = d[static_cast<long long>(yy) * Wp + xx];
    }
    __syncthreads();
    const int lx = threadIdx.x % kTileW, ly = 2 * (threadIdx.x / kTileW);
    const int x = x0 + lx;
    if (x >= w || y0 + ly >= h) return;
    float c[6][5];
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int dx = 0; dx < 5; ++dx) c[r][dx] = tile[ly + r][lx + dx];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int y = y0 + ly + j;
        if (y >= h) break;
        float m = median25(c, j);
        bool ok = m > 0.f && m < max_disp;  // range_mask (:572)
        if (conf) {
            // conf_mask = conf_mat >= threshold (:571): a float matrix against a double, compared in fp64
            const float cf = conf[win + static_cast<long long>(y) * Wp + x];
            ok = ok && static_cast<double>(cf) >= threshold;
        }
        if (!ok) m = 0.f;  // setTo(0, ~valid_mask) (:575)
        const long long o = (b * h + y) * w + x;
        if (filtered) filtered[o] = m;
        if (valid) valid[o] = ok ? 1 : 0;
        // convertTo(CV_16UC1, 256.0): saturate_cast<ushort>(d * 256) = round half to even, clamp to [0, 65535]
        const float r = rintf(m * 256.0f);
        out[o] = static_cast<uint16_t>(fminf(fmaxf(r, 0.f), 65535.f));
    }
}

// the node's own error colours (:69-92), as the bytes land in the frame: (col4, col3, col2) after COLOR_RGB2BGR,
// packed 0x00c2c1c0 like a table entry.  saturate_u8(rint((c / 255.f) * 255.f)) == c for every byte c.
constexpr int kErrRows = 10;
constexpr uint32_t kErrColour[kErrRows] = {
    149u | 54u << 8 | 49u << 16,   180u | 117u << 8 | 69u << 16,  209u | 173u << 8 | 116u << 16,
    233u | 217u << 8 | 171u << 16, 248u | 243u << 8 | 224u << 16, 144u | 224u << 8 | 254u << 16,
    97u | 174u << 8 | 253u << 16,  67u | 109u << 8 | 244u << 16,  39u | 48u << 8 | 215u << 16,
    38u | 0u << 8 | 165u << 16};
// the fp32 values of 0.1875f / 3.0f and its neighbours: row i holds kErrBound[i] <= err < kErrBound[i + 1]
constexpr float kErrBound[kErrRows + 1] = {0.0f / 3.0f,  0.1875f / 3.0f, 0.375f / 3.0f, 0.75f / 3.0f,
                                           1.5f / 3.0f,  3.0f / 3.0f,    6.0f / 3.0f,   12.0f / 3.0f,
                                           24.0f / 3.0f, 48.0f / 3.0f,   __builtin_inff()};

struct PanelArgs {
    const float* filtered;  // [B, h, w]
    const float* conf;      // [B, Hp, Wp] read through (top, left, h, w), or NULL
    const uint16_t* gt16;   // [B, h, w] or NULL
    const uint8_t* left_img;
    const uint8_t* lut;
    uint8_t* out;   // [B, 2h, 2w, 3]
    float* gt_f32;  // [B, h, w] or NULL
    int Hp, Wp, top, left, h, w;
    int groups_per_row;
    RangeRef range;
};

__global__ void __launch_bounds__(kThreads) node_panels_kernel(const PanelArgs k) {
    const int b = blockIdx.y;
    const int h = k.h, w = k.w;
    const uint32_t g = blockIdx.x * static_cast<uint32_t>(kThreads) + threadIdx.x;  // group of four pixels in a row
    const uint32_t y = g / static_cast<uint32_t>(k.groups_per_row);
    const int x0 = static_cast<int>(g - y * k.groups_per_row) * 4;
    const int n = y < static_cast<uint32_t>(h) ? min(4, w - x0) : 0;
    const long long pix = (static_cast<long long>(b) * h + y) * w + x0;
    // the loads go out first; the table and the range arrive under them
    float m[4] = {0.f, 0.f, 0.f, 0.f}, cf[4] = {0.f, 0.f, 0.f, 0.f};
    uint16_t g16[4] = {0, 0, 0, 0};
    uint32_t lb[3] = {0, 0, 0};
    if (n == 4) {
        __builtin_memcpy(m, k.filtered + pix, 16);  // element alignment, as render.hip's load_group
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) m[i] = k.filtered[pix + i];
    }
    if (k.conf) {
        const float* c = k.conf + (static_cast<long long>(b) * k.Hp + k.top + y) * k.Wp + k.left + x0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) cf[i] = c[i];
    }
    if (k.gt16) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) g16[i] = k.gt16[pix + i];
    }
    if (n) load_bytes12(k.left_img + 3 * pix, 3 * n, lb);
    __shared__ uint32_t tab[256];
    __shared__ Range part[kWaves];
    __shared__ float coef[3];
    {
        const uint8_t* e = k.lut + 3 * threadIdx.x;
        tab[threadIdx.x] = e[0] | (e[1] << 8) | (e[2] << 16);
    }
    range_coefficients(k.range, b, part, coef);
    __syncthreads();
    if (n == 0) return;
    const bool ranged = coef[2] != 0.0f;
    const float ca = ranged ? coef[0] : 0.0f, cb = ranged ? coef[1] : 0.0f;
    uint32_t disp_c[4], err_c[4], conf_c[4];
    float gt[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // bottom-left: ESM_COLORIZE_RANGE
        disp_c[i] = tab[ranged ? sat_u8(rintf(static_cast<float>(range_u(m[i])) * ca + cb)) : 0];
        // bottom-right: conf_map.convertTo(CV_8UC1, 256.0), grey (:204-205); NaN -> 0 (sat_u8)
        conf_c[i] = static_cast<uint32_t>(sat_u8(rintf(cf[i] * 256.0f))) * 0x010101u;
        // top-right: gt_mat.convertTo(CV_32FC1, 1 / 256), setTo(0, ~valid_mask) (:211-213), then vis (:94-151)
        float gv = static_cast<float>(g16[i]) * (1.0f / 256.0f);
        if (!(m[i] > 0.0f)) gv = 0.0f;
        gt[i] = gv;
        const float E = fabsf(gv - m[i]);
        const float rel = E / gv;
        const float err = rel < E ? rel : E;  // std::min(abs, rel)
        uint32_t col = 0;
#pragma unroll
        for (int r = 0; r < kErrRows; ++r)
            if (err >= kErrBound[r] && err < kErrBound[r + 1]) col = kErrColour[r];
        err_c[i] = gv > 0.0f ? col : 0u;
    }
    if (k.gt_f32) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n) k.gt_f32[pix + i] = gt[i];
    }
    const long long row = 6LL * w;  // bytes of one row of the frame
    uint8_t* tl = k.out + (static_cast<long long>(b) * 2 * h + y) * row + 3LL * x0;
    uint8_t* bl = tl + h * row;
    uint32_t r[3];
    store_group(tl, lb, 3 * n);
    pack_group(disp_c, r);
    store_group(bl, r, 3 * n);
    pack_group(err_c, r);
    store_group(tl + 3LL * w, r, 3 * n);
    pack_group(conf_c, r);
    store_group(bl + 3LL * w, r, 3 * n);
}

__global__ void __launch_bounds__(kThreads) depth16_to_disp_kernel(const uint16_t* __restrict__ depth,
                                                                   float* __restrict__ out, int Hs, int Ws, int H,
                                                                   int W, float num, float depth_scale,
                                                                   double scale_y, double scale_x, long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const int x = static_cast<int>(i % W);
    long long t = i / W;
    const int y = static_cast<int>(t % H);
    const long long b = t / H;
    // OpenCV's float INTER_LINEAR source coordinate: the double expression rounded to float, floor, fraction
    float fx = static_cast<float>((x + 0.5) * scale_x - 0.5);
    float fy = static_cast<float>((y + 0.5) * scale_y - 0.5);
    int sx = static_cast<int>(floorf(fx)), sy = static_cast<int>(floorf(fy));
    fx -= static_cast<float>(sx);
    fy -= static_cast<float>(sy);
    if (sx < 0) sx = 0, fx = 0.f;
    if (sx >= Ws - 1) sx = Ws - 1, fx = 0.f;
    if (sy < 0) sy = 0, fy = 0.f;
    if (sy >= Hs - 1) sy = Hs - 1, fy = 0.f;
    const int sx1 = min(sx + 1, Ws - 1), sy1 = min(sy + 1, Hs - 1);
    const uint16_t* src = depth + b * Hs * Ws;
    auto disp_at = [&](int yy, int xx) {
        // depthToDisparity (:69-73): z = d16 * DEPTH_SCALE; z <= 0 -> 0, else (focal * baseline) / z
        const float z = static_cast<float>(src[static_cast<long long>(yy) * Ws + xx]) * depth_scale;
        return z <= 0.0f ? 0.0f : num / z;
    };
    const float ax = 1.0f - fx, ay = 1.0f - fy;
    const float r0 = disp_at(sy, sx) * ax + disp_at(sy, sx1) * fx;
    const float r1 = disp_at(sy1, sx) * ax + disp_at(sy1, sx1) * fx;
    out[i] = r0 * ay + r1 * fy;
}

}  // namespace

int launch_node_filter_conf(const float* disp, const float* conf, uint16_t* out, float* filtered, uint8_t* valid,
                            int B, int Hp, int Wp, int top, int left, int h, int w, float max_disp, double threshold,
                            hipStream_t s) {
    if (!disp || !out) return arg_error("node_filter_conf: null pointer");
    if (B <= 0 || Hp <= 0 || Wp <= 0 || h <= 0 || w <= 0) return arg_error("node_filter_conf: non-positive size");
    if (top < 0 || left < 0 || top + h > Hp || left + w > Wp)
        return arg_error("node_filter_conf: window outside the map");
    const int tiles_x = (w + kTileW - 1) / kTileW, tiles_y = (h + kTileH - 1) / kTileH;
    const long long blocks = static_cast<long long>(B) * tiles_x * tiles_y;
    if (blocks >= (1LL << 31)) return arg_error("node_filter_conf: more than 2^31 tiles");
    hipLaunchKernelGGL(node_filter_conf_kernel, dim3(static_cast<unsigned>(blocks)), dim3(kThreads), 0, s, disp, conf,
                       out, filtered, valid, Hp, Wp, top, left, h, w, tiles_x, tiles_y, max_disp, threshold);
    return check_launch("node_filter_conf");
}

int launch_node_panels(const float* filtered, const float* conf, int Hp, int Wp, int top, int left,
                       const uint16_t* gt16, const uint8_t* left_img, const uint8_t* lut, uint8_t* out, float* gt_f32,
                       void* workspace, int B, int h, int w, hipStream_t s) {
    if (B <= 0 || h <= 0 || w <= 0 || static_cast<long long>(h) * w >= (1LL << 31))
        return arg_error("node_panels: sizes must be positive and h * w below 2^31");
    if (!filtered || !left_img || !lut || !out || !workspace) return arg_error("node_panels: null pointer");
    if (B > 65535) return arg_error("node_panels: batch above 65535");
    if (conf) {
        if (Hp <= 0 || Wp <= 0) return arg_error("node_panels: non-positive size of the confidence map");
        if (top < 0 || left < 0 || top + h > Hp || left + w > Wp)
            return arg_error("node_panels: window outside the confidence map");
    }
    PanelArgs k = {};
    k.filtered = filtered, k.conf = conf, k.gt16 = gt16, k.left_img = left_img, k.lut = lut, k.out = out;
    k.gt_f32 = gt_f32;
    k.Hp = Hp, k.Wp = Wp, k.top = top, k.left = left, k.h = h, k.w = w;
    k.groups_per_row = (w + 3) / 4;
    if (int rc = launch_range_pass(filtered, static_cast<long long>(h) * w, w, B, h, w, workspace, s, &k.range))
        return rc;
    const long long groups = static_cast<long long>(h) * k.groups_per_row;
    hipLaunchKernelGGL(node_panels_kernel, dim3(ceil_div(groups, kThreads), B), dim3(kThreads), 0, s, k);
    return check_launch("node_panels");
}

int launch_depth16_to_disp(const uint16_t* depth, float* out, int B, int Hs, int Ws, int H, int W, float num,
                           float depth_scale, hipStream_t s) {
    if (!depth || !out) return arg_error("depth16_to_disp: null pointer");
    if (B <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0) return arg_error("depth16_to_disp: non-positive size");
    if (static_cast<long long>(Hs) * Ws >= (1LL << 31) || static_cast<long long>(H) * W >= (1LL << 31))
        return arg_error("depth16_to_disp: H * W must be below 2^31");
    const long long n = static_cast<long long>(B) * H * W;
    if ((n + kThreads - 1) / kThreads >= (1LL << 31)) return arg_error("depth16_to_disp: batch too large");
    const double scale_x = static_cast<double>(Ws) / W, scale_y = static_cast<double>(Hs) / H;
    hipLaunchKernelGGL(depth16_to_disp_kernel, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, depth, out, Hs, Ws, H,
                       W, num, depth_scale, scale_y, scale_x, n);
    return check_launch("depth16_to_disp");
}

}  // namespace esm

extern "C" {

int esm_node_filter_conf_u16(const float* disp, const float* conf, uint16_t* out, float* filtered, uint8_t* valid,
                             int B, int Hp, int Wp, int top, int left, int h, int w, float max_disp,
                             double threshold, void* stream) {
    return esm::launch_node_filter_conf(disp, conf, out, filtered, valid, B, Hp, Wp, top, left, h, w, max_disp,
                                        threshold, esm::as_stream(stream));
}

int esm_node_panels_u8(const float* filtered, const float* conf, int Hp, int Wp, int top, int left,
                       const uint16_t* gt16, const uint8_t* left_img, const uint8_t* lut, uint8_t* out, float* gt_f32,
                       void* workspace, int B, int h, int w, void* stream) {
    return esm::launch_node_panels(filtered, conf, Hp, Wp, top, left, gt16, left_img, lut, out, gt_f32, workspace, B,
                                   h, w, esm::as_stream(stream));
}

int esm_depth16_to_disp_f32(const uint16_t* depth16, float* out, int B, int Hs, int Ws, int H, int W, float num,
                            float depth_scale, void* stream) {
    return esm::launch_depth16_to_disp(depth16, out, B, Hs, Ws, H, W, num, depth_scale, esm::as_stream(stream));
}

}  // extern "C"
