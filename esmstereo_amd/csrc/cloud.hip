// Point clouds on the device: the 3-D points of a disparity map, reprojected through a rectified pinhole camera,
// compacted in raster order and coloured, as one plan op (esm_plan_add_cloud; the definition is esm_cloud_desc's
// comment in include/esmstereo_amd.h).  The reference node has the camera (kitti_publisher_cuda_node.cpp:60-78,
// 277-278) and latest.py:54-58 the depth; the points themselves are what a consumer of either builds next.
//
// Shape.  A per-pixel map and an order-preserving stream compaction: 4 B read per candidate (7-8 B more for a kept
// coloured one) and 12 or 16 B written per kept point.  The candidates of an image (the pixels with x % step == 0 and
// y % step == 0, in raster order) are cut into tiles of kTile = 2048; three stream-ordered launches, the whole batch
// in each, no host synchronisation:
//   1 cloud_count_kernel  one workgroup per tile: the keep flags, their number -> work[b, tile] (a plain store).
//   2 cloud_scan_kernel   one workgroup per image: the tile counts scanned in place into tile offsets, 256 at a time
//                         with a carry between rounds (jpeg_scan_kernel's form); counts[b].
//   3 cloud_emit_kernel   one workgroup per tile: the flags and the points again (three divisions and two multiplies
//                         against 13-17 B per candidate parked in a workspace), each lane's rank in the tile, the
//                         records staged in LDS at their rank, then written from record work[b, tile] of the image's
//                         slot as coalesced stores: dwordx4 for 16-byte records, dwords for 12-byte ones.
// No workgroup waits on another: the three launches are the ordering.  A single-pass compaction (decoupled look-back)
// would save one read of the map (an estimate, not a measurement: 1.9 MB of a 375 x 1242 map, well under a
// microsecond at HBM rate) and the scan launch, and spins on flags other workgroups write; a workgroup that is never
// scheduled behind the spinning ones hangs the device for everybody on it.
// Thread t of a tile takes candidates j * 256 + t, j < 8, so a wave's loads are consecutive (step 1) and the raster
// order is (j, wave, lane): a lane's rank is the kept lanes below it in its wave's ballot, plus the ballots' popcounts
// of the (j, wave) pairs in front, 32 words of LDS every lane sums as broadcast reads.
// LDS: 2048 records of 16 B = 32,768 B staging + 128 B counts: four workgroups per CU of 163,840 B.  The staging
// writes are at consecutive ranks within a wave (the kept lanes), 16 B (or 12 B, an odd dword stride) apart: no two
// lanes of a group share a bank; the reads back are consecutive 16-byte (4-byte) cells per lane.
// The offsets pass through LDS and the workspace, so every staging index is compared with kTile and every record
// index with slot_points before the store (the png.hip convention).
#include <cmath>

#include "common.h"
#include "scan.h"

// every operation rounded once, as numpy rounds it
#pragma clang fp contract(off)

namespace esm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPer = 8;                   // candidates per thread
constexpr int kTile = kThreads * kPer;    // 2048 candidates per workgroup

struct CloudArgs {
    const float* disp;
    long long sb, sh;
    const uint8_t* color;
    const uint8_t* valid;
    uint8_t* out;
    long long slot;    // records per image slot
    int32_t* counts;
    uint32_t* work;    // [B, tiles]: tile counts, then (in place) tile offsets
    int H, W, step, Ws;
    uint32_t ncand;    // candidates per image, < 2^31
    int tiles, bgr, packing;
    float num, fx, fy, cx, cy, z_min, z_max;
};

struct Point {
    float x, y, z;
    uint32_t pix;  // y * W + x
};

// candidate c of image b: its point, and whether it is kept
__device__ __forceinline__ bool candidate(const CloudArgs& k, int b, uint32_t c, Point& p) {
    p = {0.0f, 0.0f, 0.0f, 0u};
    if (c >= k.ncand) return false;
    const uint32_t ys = c / static_cast<uint32_t>(k.Ws);
    const uint32_t xs = c - ys * static_cast<uint32_t>(k.Ws);
    const uint32_t y = ys * static_cast<uint32_t>(k.step), x = xs * static_cast<uint32_t>(k.step);
    p.pix = y * static_cast<uint32_t>(k.W) + x;
    const float d = k.disp[b * k.sb + y * k.sh + x];
    p.z = k.num / d;
    p.x = (static_cast<float>(x) - k.cx) * p.z / k.fx;
    p.y = (static_cast<float>(y) - k.cy) * p.z / k.fy;
    bool keep = d > 0.0f && p.z >= k.z_min && p.z <= k.z_max;  // a NaN fails every comparison
    if (keep && k.valid) keep = k.valid[static_cast<long long>(b) * k.H * k.W + p.pix] != 0;
    return keep;
}

__global__ void __launch_bounds__(kThreads) cloud_count_kernel(const CloudArgs k) {
    const int b = blockIdx.y;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        Point p;
        n += candidate(k, b, blockIdx.x * static_cast<uint32_t>(kTile) + j * kThreads + threadIdx.x, p) ? 1u : 0u;
    }
    __shared__ uint32_t wsum[kWaves];
    n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += wsum[w];
        k.work[static_cast<long long>(b) * k.tiles + blockIdx.x] = t;
    }
}

// one workgroup per image: its tile counts -> tile offsets, in place; counts[b].  An image has fewer than 2^31
// candidates, so every sum fits 32 bits.
__global__ void __launch_bounds__(kThreads) cloud_scan_kernel(const CloudArgs k) {
    __shared__ uint32_t wsum[kWaves];
    const long long b = blockIdx.x;
    uint32_t* w = k.work + b * k.tiles;
    uint32_t carry = 0;
    for (int c0 = 0; c0 < k.tiles; c0 += kThreads) {
        const int c = c0 + threadIdx.x;
        const uint32_t n = c < k.tiles ? w[c] : 0;
        uint32_t total;
        const uint32_t off = block_scan<kThreads>(n, wsum, total);
        if (c < k.tiles) w[c] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) k.counts[b] = static_cast<int32_t>(carry);
}

template <bool COLOR>
__global__ void __launch_bounds__(kThreads) cloud_emit_kernel(const CloudArgs k) {
    constexpr int kRec = COLOR ? 4 : 3;  // dwords per record
    __shared__ __attribute__((aligned(16))) uint32_t stage[kTile * kRec];
    __shared__ __attribute__((aligned(16))) uint32_t wcount[kPer * kWaves];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Point p[kPer];
    bool keep[kPer];
    uint32_t rank[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        keep[j] = candidate(k, b, blockIdx.x * static_cast<uint32_t>(kTile) + j * kThreads + threadIdx.x, p[j]);
        const unsigned long long m = __ballot(keep[j]);
        rank[j] = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(m >> 32),
                                            __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0u));
        if (lane == 0) wcount[j * kWaves + wave] = static_cast<uint32_t>(__popcll(m));
    }
    __syncthreads();
    uint32_t n = 0;  // kept in the (j, wave) pairs in front; at the end the tile's count
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        uint32_t c[kWaves];
        __builtin_memcpy(c, wcount + j * kWaves, sizeof(c));
        rank[j] += n + (wave > 0 ? c[0] : 0u) + (wave > 1 ? c[1] : 0u) + (wave > 2 ? c[2] : 0u);
        n += c[0] + c[1] + c[2] + c[3];
    }
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        if (!keep[j] || rank[j] >= static_cast<uint32_t>(kTile)) continue;
        uint32_t r[4] = {__float_as_uint(p[j].x), __float_as_uint(p[j].y), __float_as_uint(p[j].z), 0u};
        if constexpr (COLOR) {
            const uint8_t* s = k.color + (static_cast<long long>(b) * k.H * k.W + p[j].pix) * 3;
            const uint32_t c0 = s[0], c1 = s[1], c2 = s[2];
            const uint32_t red = k.bgr ? c2 : c0, blue = k.bgr ? c0 : c2;
            r[3] = k.packing == ESM_CLOUD_PACK_PLY ? (red | c1 << 8 | blue << 16 | 255u << 24)
                                                   : (blue | c1 << 8 | red << 16);
            __builtin_memcpy(stage + rank[j] * 4, r, 16);
        } else {
            __builtin_memcpy(stage + rank[j] * 3, r, 12);
        }
    }
    __syncthreads();
    n = min(n, static_cast<uint32_t>(kTile));
    if (n == 0) return;
    const long long first = k.work[static_cast<long long>(b) * k.tiles + blockIdx.x];  // record index in the slot
    const long long base = static_cast<long long>(b) * k.slot + first;                 // ... and in `out`
    if constexpr (COLOR) {
        uint4* dst = reinterpret_cast<uint4*>(k.out) + base;
        const uint4* src = reinterpret_cast<const uint4*>(stage);
        for (uint32_t i = threadIdx.x; i < n; i += kThreads)
            if (first + i < k.slot) dst[i] = src[i];
    } else {
        uint32_t* dst = reinterpret_cast<uint32_t*>(k.out) + base * 3;
        for (uint32_t i = threadIdx.x; i < 3 * n; i += kThreads)
            if (first * 3 + i < k.slot * 3) dst[i] = stage[i];
    }
}

bool size_ok(int H, int W, int step) {
    return H > 0 && W > 0 && step > 0 && static_cast<long long>(H) * W < (1LL << 31);
}

long long sampled(int n, int step) { return (static_cast<long long>(n) + step - 1) / step; }

long long tiles_of(int H, int W, int step) { return (sampled(H, step) * sampled(W, step) + kTile - 1) / kTile; }

}  // namespace

long long cloud_max_points(int H, int W, int step) {
    if (!size_ok(H, W, step)) return arg_error("cloud_max_points: sizes and step must be positive and H * W below 2^31");
    return sampled(H, step) * sampled(W, step);
}

long long cloud_workspace_bytes(int B, int H, int W, int step) {
    if (B <= 0 || !size_ok(H, W, step))
        return arg_error("cloud_workspace_bytes: sizes and step must be positive and H * W below 2^31");
    if (B > 65535) return arg_error("cloud_workspace_bytes: batch above 65535");
    return static_cast<long long>(B) * tiles_of(H, W, step) * static_cast<long long>(sizeof(uint32_t));
}

// The record size of an acceptable descriptor (12 or 16), or ESM_ERR_ARG: decided on the descriptor's own words, before
// any pointer is followed and before any HIP call.
int cloud_check(const esm_cloud_desc* d) {
    if (!d) return arg_error("cloud: null descriptor");
    if (!d->disp || !d->out || !d->counts || !d->work) return arg_error("cloud: null disp / out / counts / work");
    if (d->B <= 0 || d->H <= 0 || d->W <= 0 || d->step <= 0) return arg_error("cloud: sizes and step must be positive");
    if (d->disp_sb < 0 || d->disp_sh < 0) return arg_error("cloud: negative stride");
    if (d->B > 65535) return arg_error("cloud: batch above 65535");
    if (static_cast<long long>(d->H) * d->W >= (1LL << 31)) return arg_error("cloud: H * W must be below 2^31");
    if (reinterpret_cast<uintptr_t>(d->disp) % 4 || reinterpret_cast<uintptr_t>(d->out) % 16 ||
        reinterpret_cast<uintptr_t>(d->counts) % 4 || reinterpret_cast<uintptr_t>(d->work) % 4)
        return arg_error("cloud: disp, counts and work must be 4-byte aligned, out 16-byte aligned");
    if (d->packing != ESM_CLOUD_PACK_PLY && d->packing != ESM_CLOUD_PACK_PCL) return arg_error("cloud: unknown packing");
    if (!std::isfinite(d->fx) || !std::isfinite(d->fy) || d->fx == 0.0f || d->fy == 0.0f)
        return arg_error("cloud: fx and fy must be finite and not zero");
    if (!(d->z_min <= d->z_max)) return arg_error("cloud: z_min above z_max, or a NaN bound");
    if (d->slot_points < cloud_max_points(d->H, d->W, d->step))
        return arg_error("cloud: slot_points below esm_cloud_max_points(H, W, step)");
    const long long rec = d->color ? 16 : 12;
    const long long per = static_cast<long long>(d->B) * rec;
    if (d->slot_points >= ((1LL << 40) + per - 1) / per) return arg_error("cloud: B * slot_points * record bytes reaches 2^40");
    return static_cast<int>(rec);
}

int launch_cloud(const esm_cloud_desc* d, hipStream_t s) {
    const int rec = cloud_check(d);
    if (rec < 0) return rec;
    CloudArgs k = {};
    k.disp = d->disp, k.sb = d->disp_sb, k.sh = d->disp_sh;
    k.color = d->color, k.valid = d->valid;
    k.out = static_cast<uint8_t*>(d->out), k.slot = d->slot_points;
    k.counts = d->counts, k.work = static_cast<uint32_t*>(d->work);
    k.H = d->H, k.W = d->W, k.step = d->step, k.Ws = static_cast<int>(sampled(d->W, d->step));
    k.ncand = static_cast<uint32_t>(cloud_max_points(d->H, d->W, d->step));
    k.tiles = static_cast<int>(tiles_of(d->H, d->W, d->step));
    k.bgr = d->bgr != 0, k.packing = d->packing;
    k.num = d->num, k.fx = d->fx, k.fy = d->fy, k.cx = d->cx, k.cy = d->cy, k.z_min = d->z_min, k.z_max = d->z_max;
    const dim3 grid(k.tiles, d->B), block(kThreads);
    hipLaunchKernelGGL(cloud_count_kernel, grid, block, 0, s, k);
    if (int rc = check_launch("cloud (count)")) return rc;
    hipLaunchKernelGGL(cloud_scan_kernel, dim3(d->B), block, 0, s, k);
    if (int rc = check_launch("cloud (scan)")) return rc;
    if (rec == 16)
        hipLaunchKernelGGL(cloud_emit_kernel<true>, grid, block, 0, s, k);
    else
        hipLaunchKernelGGL(cloud_emit_kernel<false>, grid, block, 0, s, k);
    return check_launch("cloud (emit)");
}

}  // namespace esm

extern "C" {

int esm_cloud_tile_points(void) { return esm::kTile; }

long long esm_cloud_max_points(int H, int W, int step) { return esm::cloud_max_points(H, W, step); }

long long esm_cloud_workspace_bytes(int B, int H, int W, int step) { return esm::cloud_workspace_bytes(B, H, W, step); }

int esm_cloud_check(const esm_cloud_desc* desc) { return esm::cloud_check(desc); }

}  // extern "C"
