// What render.hip (esm_disp_colorize_u8) and node_conf.hip (esm_node_panels_u8) share: the RANGE definition of a
// pixel's table index (u, the per-image integer range, the coefficients a and b), the pass that finds the range,
// and the 12-byte group stores of a colour row.  One definition, so the four-panel frame's colour panel is
// ESM_COLORIZE_RANGE by construction.
#pragma once

#include "common.h"

namespace esm {
namespace rdr {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct Range {
    uint32_t mn, mx;  // of u over the valid pixels; mn > mx: there is none
};
static_assert(sizeof(Range) == 8, "workspace record");

// where the range pass left image b's partials: ranges + b * stride, n of them
struct RangeRef {
    const Range* ranges;
    int n, stride;
};

__device__ __forceinline__ int sat_u8(float r) { return static_cast<int>(fminf(fmaxf(r, 0.0f), 255.0f)); }

__device__ __forceinline__ uint32_t range_u(float m) {
    return m > 0.0f ? static_cast<uint32_t>(fminf(rintf(m * 256.0f), 65535.0f)) : 0u;
}

__device__ __forceinline__ Range merge(Range a, Range b) { return {min(a.mn, b.mn), max(a.mx, b.mx)}; }

// every thread returns the workgroup's range (one use per kernel: `part` is not reused)
__device__ __forceinline__ Range block_range(Range r, Range (&part)[kWaves]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) r = merge(r, Range{__shfl_xor(r.mn, d), __shfl_xor(r.mx, d)});
    if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = r;
    __syncthreads();
    r = part[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = merge(r, part[w]);
    return r;
}

// Image b's partials -> coef = {a, b, whether the image has a range at all}, written by thread 0; the caller's
// __syncthreads() publishes it.  a and b in fp64, each rounded once.
__device__ __forceinline__ void range_coefficients(const RangeRef& k, int b, Range (&part)[kWaves], float (&coef)[3]) {
    const Range* pr = k.ranges + static_cast<long long>(b) * k.stride;
    Range r = {0xFFFFFFFFu, 0u};
    for (int t = threadIdx.x; t < k.n; t += kThreads) r = merge(r, pr[t]);
    r = block_range(r, part);
    if (threadIdx.x == 0) {
        const bool ok = r.mn < r.mx;
        const double span = static_cast<double>(r.mx) - static_cast<double>(r.mn);
        coef[0] = ok ? static_cast<float>(-255.0 / span) : 0.0f;
        coef[1] = ok ? static_cast<float>(255.0 * static_cast<double>(r.mx) / span) : 0.0f;
        coef[2] = ok ? 1.0f : 0.0f;
    }
}

// nbytes <= 12 bytes, the little-endian contents of r[0..2], to o.  Vector stores only.
__device__ __forceinline__ void store_group(uint8_t* __restrict__ o, const uint32_t (&r)[3], int nbytes) {
    const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(o) & 3);
    if (nbytes == 12 && mis == 0) {
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
        o4[0] = r[0];
        o4[1] = r[1];
        o4[2] = r[2];
    } else if (nbytes == 12) {
        const int hc = 4 - mis, s = 8 * hc;  // leading bytes up to the next aligned dword; 8 <= s <= 24
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < hc) o[i] = static_cast<uint8_t>(r[0] >> (8 * i));
        uint32_t* o4 = reinterpret_cast<uint32_t*>(o + hc);
        o4[0] = (r[0] >> s) | (r[1] << (32 - s));
        o4[1] = (r[1] >> s) | (r[2] << (32 - s));
        const uint32_t t = r[2] >> s;
#pragma unroll
        for (int i = 0; i < 3; ++i)
            if (i < mis) o[hc + 8 + i] = static_cast<uint8_t>(t >> (8 * i));
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < nbytes) o[i] = static_cast<uint8_t>(r[i / 4] >> (8 * (i % 4)));
    }
}

// nbytes <= 12 bytes from s into r[0..2], little-endian; the rest of r is 0
__device__ __forceinline__ void load_bytes12(const uint8_t* __restrict__ s, int nbytes, uint32_t (&r)[3]) {
    r[0] = r[1] = r[2] = 0;
    if (nbytes == 12 && (reinterpret_cast<uintptr_t>(s) & 3) == 0) {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
        r[0] = s4[0], r[1] = s4[1], r[2] = s4[2];
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            if (i < nbytes) r[i / 4] |= static_cast<uint32_t>(s[i]) << (8 * (i % 4));
    }
}

// four packed table entries (0x00c2c1c0 each) -> the 12 bytes of four pixels
__device__ __forceinline__ void pack_group(const uint32_t (&c)[4], uint32_t (&r)[3]) {
    r[0] = c[0] | (c[1] << 24);
    r[1] = (c[1] >> 8) | (c[2] << 16);
    r[2] = (c[2] >> 16) | (c[3] << 8);
}

}  // namespace rdr

// The range pass of ESM_COLORIZE_RANGE over disp [B, H, W] (batch and row strides in elements), defined in
// render.hip: one or two launches on s, partials in `workspace` (esm_disp_colorize_workspace(B, H, W) bytes).
// The sizes are the caller's to check (positive, H * W < 2^31, B <= 65535).
int launch_range_pass(const float* disp, long long sb, long long sh, int B, int H, int W, void* workspace,
                      hipStream_t s, rdr::RangeRef* where);

}  // namespace esm
