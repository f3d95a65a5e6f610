// Scoring a disparity against ground truth on the device (utils/metrics.py, utils/visualization.py):
//
//  esm_disp_metrics_f32   EPE_metric, D1_metric, D1_metric_thres and Thres_metric (utils/metrics.py:42-74) with
//    the per-image skip rule and batch mean of compute_metric_for_each_image (:17-39), for up to four
//    thresholds at once, in one pass over est, gt and mask.  The reference compacts est[mask] and gt[mask]
//    per image and per metric (two boolean-index kernels and a host sync each) and syncs twice more for the
//    skip rule; here nothing is compacted and the host never waits.
//      E       = |gt - est|                         one fp32 operation
//      EPE     = mean(E[mask])                      fp64 sum / count, rounded once to fp32
//      Thres_t = mean(E[mask] > t)                  float(count) / float(n_mask): the bits of torch's
//      D1_t    = mean((E > t) & (E / |gt| > rel))   fp32 mean of a 0/1 tensor below 2^24 elements
//      skipped = mean(mask) / mean(gt > 0) < 0.1f   fp32; 0/0 = NaN is not < 0.1, the image is kept
//    Values are selected by the mask, never multiplied by it: a NaN outside the mask reaches nothing.
//    Two launches: metrics_partial_kernel (one fixed-order partial record per workgroup) and
//    metrics_final_kernel (per-image records and values, then the batch means).  No float atomics: every
//    sum has a fixed order, so two runs give the same bits.
//  esm_disp_error_map_f32  the KITTI error image `vis` (utils/visualization.py:20-37): one thread per pixel,
//    three coalesced plane stores, IEEE divisions (a multiply by a reciprocal gives other bits).
//
// Inputs are addressed by (batch stride, row stride) in elements, W contiguous, so the crop
// pred[:, hi-h:, wi-w:] of a padded output (test_kitti.py:114) is read where it lies.
// All of it is HBM-bound: (4 + 4 + 1) H W bytes per image for the metrics (8 without a mask tensor), 8 H W read
// and 12 H W written for the error map; at KITTI size (0.47 Mpx) both are launch-latency-bound.
#include "common.h"
#include "scan.h"

// every operation rounded once, as torch / numpy round it
#pragma clang fp contract(off)

namespace esm {
namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQuadsPerThread = 4;
constexpr int kTileQuads = kThreads * kQuadsPerThread;  // 4096 pixels per workgroup
constexpr int kMaxThres = ESM_METRICS_MAX_THRES;
constexpr int kCounts = 2 + 2 * kMaxThres;  // n_mask, n_gt_pos, n_abs[4], n_both[4]
constexpr int kRecord = ESM_METRICS_RECORD_DOUBLES;
constexpr int kValues = ESM_METRICS_VALUES;

struct Partial {
    double sum;
    uint32_t cnt[kCounts];
};
static_assert(sizeof(Partial) == ESM_METRICS_PARTIAL_BYTES, "partial record size is part of the ABI");
static_assert(kRecord == 4 + 2 * kMaxThres && kValues == 2 + 2 * kMaxThres, "record layouts");

struct View {
    const void* p;
    long long sb, sh;
};

struct MetricArgs {
    View est, gt, mask;
    int H, W, Wq, tiles;
    float lo, hi;
    int use_range, nthres;
    float thres[kMaxThres];
    float rel;
};

struct Acc {
    double sum = 0.0;
    uint32_t cnt[kCounts] = {};
};

__device__ __forceinline__ void score(Acc& a, const MetricArgs& k, float est, float gt, bool m) {
    a.cnt[1] += gt > 0.0f;
    if (k.use_range) m = m && gt > k.lo && gt < k.hi;
    const float e = fabsf(gt - est);
    const bool rel = e / fabsf(gt) > k.rel;
    a.cnt[0] += m;
    a.sum += m ? static_cast<double>(e) : 0.0;
#pragma unroll
    for (int t = 0; t < kMaxThres; ++t) {
        const bool over = m && t < k.nthres && e > k.thres[t];
        a.cnt[2 + t] += over;
        a.cnt[2 + kMaxThres + t] += over && rel;
    }
}

__global__ void __launch_bounds__(kThreads) metrics_partial_kernel(const MetricArgs k, Partial* __restrict__ ws) {
    const int b = blockIdx.y;
    const float* est = static_cast<const float*>(k.est.p) + b * k.est.sb;
    const float* gt = static_cast<const float*>(k.gt.p) + b * k.gt.sb;
    const uint8_t* mask = k.mask.p ? static_cast<const uint8_t*>(k.mask.p) + b * k.mask.sb : nullptr;
    const long long nq = static_cast<long long>(k.H) * k.Wq;
    // every load of the thread's four groups is issued before anything is scored: a group past the end re-reads
    // the image's last group (in bounds) and is not scored
    float e[kQuadsPerThread][4], g[kQuadsPerThread][4];
    uint8_t m[kQuadsPerThread][4];
    int n[kQuadsPerThread];
#pragma unroll
    for (int j = 0; j < kQuadsPerThread; ++j) {
        const long long q = static_cast<long long>(blockIdx.x) * kTileQuads + j * kThreads + threadIdx.x;
        const long long qc = min(q, nq - 1);
        const int y = static_cast<int>(qc / k.Wq);
        const int x = static_cast<int>(qc - static_cast<long long>(y) * k.Wq) * 4;
        const int w = min(4, k.W - x);  // < 4 in a row's tail
        n[j] = q < nq ? w : 0;
        const float* pe = est + y * k.est.sh + x;
        const float* pg = gt + y * k.gt.sh + x;
        const uint8_t* pm = mask ? mask + y * k.mask.sh + x : nullptr;
        if (w == 4) {
            // 16 bytes (mask: 4) in one load.  Only element alignment is assumed, which gfx950's global loads
            // need and no more: a crop's rows start anywhere, and a group that straddles two cache lines costs a
            // second access, not a fault.
            __builtin_memcpy(e[j], pe, 16);
            __builtin_memcpy(g[j], pg, 16);
            if (pm) __builtin_memcpy(m[j], pm, 4);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                e[j][i] = i < w ? pe[i] : 0.0f;
                g[j][i] = i < w ? pg[i] : 0.0f;
                if (pm) m[j][i] = i < w ? pm[i] : 0;
            }
        }
        if (!pm) m[j][0] = m[j][1] = m[j][2] = m[j][3] = 1;
    }
    Acc a;
#pragma unroll
    for (int j = 0; j < kQuadsPerThread; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < n[j]) score(a, k, e[j][i], g[j][i], m[j][i] != 0);
    // across the wave: xor butterfly (every lane ends with the same bits), then the waves in index order
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        a.sum += __shfl_xor(a.sum, d);
#pragma unroll
        for (int c = 0; c < kCounts; ++c) a.cnt[c] += __shfl_xor(a.cnt[c], d);
    }
    __shared__ Partial part[kWaves];
    const int wave = threadIdx.x / 64;
    if (threadIdx.x % 64 == 0) {
        part[wave].sum = a.sum;
#pragma unroll
        for (int c = 0; c < kCounts; ++c) part[wave].cnt[c] = a.cnt[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial r = part[0];
        for (int w = 1; w < kWaves; ++w) {
            r.sum += part[w].sum;
#pragma unroll
            for (int c = 0; c < kCounts; ++c) r.cnt[c] += part[w].cnt[c];
        }
        ws[static_cast<long long>(b) * k.tiles + blockIdx.x] = r;
    }
}

// One workgroup.  Wave w finishes images w, w + kWaves, ...: 64 partials at a time are loaded side by side and
// added lane after lane, i.e. in index order.  Then one thread per value forms the batch means in image order.
__global__ void __launch_bounds__(kThreads) metrics_final_kernel(const Partial* __restrict__ ws, int B, int tiles,
                                                                 int npix, int nthres, double* __restrict__ records,
                                                                 float* values, float* __restrict__ batch) {
    const int lane = threadIdx.x % 64;
    for (int b = threadIdx.x / 64; b < B; b += kWaves) {
        const Partial* p = ws + static_cast<long long>(b) * tiles;
        double sum = 0.0;
        unsigned long long cnt[kCounts] = {};
        for (int t0 = 0; t0 < tiles; t0 += 64) {
            Partial v = {};
            if (t0 + lane < tiles) v = p[t0 + lane];
            // lanes past the last partial hold +0.0, which changes no sum (the terms are >= 0 or NaN): all 64
            // lanes are read, each through v_readlane with a constant index (a shuffle by a loop variable is a
            // dependent LDS round trip per term: this kernel took 8.3 us that way and 4.7 us this way, at 114
            // and at 8 x 128 partials)
#pragma unroll
            for (int l = 0; l < 64; ++l)
                sum += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v.sum), l),
                                        __builtin_amdgcn_readlane(__double2loint(v.sum), l));
#pragma unroll
            for (int c = 0; c < kCounts; ++c)
                cnt[c] += wave_sum(v.cnt[c]);  // (32 bits: an image has fewer than 2^31 pixels)
        }
        if (lane == 0) {
            double* r = records + static_cast<long long>(b) * kRecord;
            r[0] = static_cast<double>(cnt[0]);
            r[1] = static_cast<double>(cnt[1]);
            r[2] = sum;
            r[3] = 0.0;
            for (int c = 2; c < kCounts; ++c) r[2 + c] = static_cast<double>(cnt[c]);
            float* v = values + static_cast<long long>(b) * kValues;
            const float nm = static_cast<float>(cnt[0]);
            v[0] = static_cast<float>(sum / static_cast<double>(cnt[0]));
            for (int t = 0; t < kMaxThres; ++t) {
                v[1 + t] = t < nthres ? static_cast<float>(cnt[2 + t]) / nm : 0.0f;
                v[1 + kMaxThres + t] = t < nthres ? static_cast<float>(cnt[2 + kMaxThres + t]) / nm : 0.0f;
            }
            // masks[idx].float().mean() / (D_gts[idx] > 0).float().mean() < 0.1 (utils/metrics.py:26)
            const float fn = static_cast<float>(npix);
            const float ratio = (nm / fn) / (static_cast<float>(cnt[1]) / fn);
            v[kValues - 1] = ratio < 0.1f ? 1.0f : 0.0f;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < kValues - 1) {
        // torch.stack(kept).mean(), or 0 when nothing is kept (utils/metrics.py:31-37)
        float s = 0.0f;
        int kept = 0;
        for (int b = 0; b < B; ++b) {
            const volatile float* v = values + static_cast<long long>(b) * kValues;
            if (v[kValues - 1] != 0.0f) continue;
            s += v[threadIdx.x];
            ++kept;
        }
        batch[threadIdx.x] = kept ? s / static_cast<float>(kept) : 0.0f;
        if (threadIdx.x == 0) batch[kValues - 1] = static_cast<float>(kept);
    }
}

// utils/visualization.py:4-18: bounds float32(x / 3.0), colours float32(c) / float32(255)
constexpr int kBuckets = 10;
__constant__ const float kBound[kBuckets + 1] = {
    static_cast<float>(0 / 3.0),  static_cast<float>(0.1875 / 3.0), static_cast<float>(0.375 / 3.0),
    static_cast<float>(0.75 / 3.0), static_cast<float>(1.5 / 3.0),  static_cast<float>(3 / 3.0),
    static_cast<float>(6 / 3.0),  static_cast<float>(12 / 3.0),     static_cast<float>(24 / 3.0),
    static_cast<float>(48 / 3.0), __builtin_huge_valf()};
__constant__ const float kColour[kBuckets][3] = {
    {49.f / 255.f, 54.f / 255.f, 149.f / 255.f},   {69.f / 255.f, 117.f / 255.f, 180.f / 255.f},
    {116.f / 255.f, 173.f / 255.f, 209.f / 255.f}, {171.f / 255.f, 217.f / 255.f, 233.f / 255.f},
    {224.f / 255.f, 243.f / 255.f, 248.f / 255.f}, {254.f / 255.f, 224.f / 255.f, 144.f / 255.f},
    {253.f / 255.f, 174.f / 255.f, 97.f / 255.f},  {244.f / 255.f, 109.f / 255.f, 67.f / 255.f},
    {215.f / 255.f, 48.f / 255.f, 39.f / 255.f},   {165.f / 255.f, 0.f / 255.f, 38.f / 255.f}};

__global__ void __launch_bounds__(kThreads) error_map_kernel(const float* __restrict__ est, long long eb,
                                                             long long eh, const float* __restrict__ gt,
                                                             long long gb, long long gh, float* __restrict__ out,
                                                             int H, int W, float abs_thres, float rel_thres,
                                                             long long n) {
    const long long i = static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const long long plane = static_cast<long long>(H) * W;
    const long long b = i / plane;
    const long long r = i - b * plane;
    const int y = static_cast<int>(r / W);
    const int x = static_cast<int>(r - static_cast<long long>(y) * W);
    int bucket = -1;
    if (y < 10 && x < 20 * kBuckets) {
        bucket = x / 20;  // the legend, written last in the reference: over the mask as well
    } else {
        const float g = gt[b * gb + y * gh + x];
        if (g > 0.0f) {
            const float e = fabsf(g - est[b * eb + y * eh + x]);
            const float ea = e / abs_thres, er = (e / g) / rel_thres;
            const float err = (ea <= er || ea != ea) ? ea : er;  // np.minimum: a NaN wins
#pragma unroll
            for (int c = 0; c < kBuckets; ++c)
                if (err >= kBound[c] && err < kBound[c + 1]) bucket = c;
        }
    }
    float* o = out + b * 3 * plane + r;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c * plane] = bucket >= 0 ? kColour[bucket][c] : 0.0f;
}

bool size_ok(int B, int H, int W) {
    return B > 0 && H > 0 && W > 0 && static_cast<long long>(H) * W < (1LL << 31);
}

long long tiles_of(int H, int W) {
    const long long nq = static_cast<long long>(H) * ((W + 3) / 4);
    return (nq + kTileQuads - 1) / kTileQuads;
}

}  // namespace

long long metrics_workspace(int B, int H, int W) {
    if (!size_ok(B, H, W)) return arg_error("disp_metrics_workspace: sizes must be positive and H * W below 2^31");
    return static_cast<long long>(B) * tiles_of(H, W) * static_cast<long long>(sizeof(Partial));
}

int launch_metrics(const float* est, long long eb, long long eh, const float* gt, long long gb, long long gh,
                   const uint8_t* mask, long long mb, long long mh, int B, int H, int W, float lo, float hi,
                   int use_range, const float* thres, int nthres, float rel, void* workspace, double* records,
                   float* values, float* batch, hipStream_t s) {
    if (!size_ok(B, H, W)) return arg_error("disp_metrics: sizes must be positive and H * W below 2^31");
    if (!est || !gt || !workspace || !records || !values || !batch) return arg_error("disp_metrics: null pointer");
    if (nthres < 0 || nthres > kMaxThres || (nthres > 0 && !thres))
        return arg_error("disp_metrics: 0..4 thresholds, thres non-null when there are any");
    if (eb < 0 || eh < 0 || gb < 0 || gh < 0 || mb < 0 || mh < 0) return arg_error("disp_metrics: negative stride");
    if (B > 65535) return arg_error("disp_metrics: batch above 65535");
    MetricArgs k = {};
    k.est = {est, eb, eh};
    k.gt = {gt, gb, gh};
    k.mask = {mask, mb, mh};
    k.H = H, k.W = W, k.Wq = (W + 3) / 4;
    k.tiles = static_cast<int>(tiles_of(H, W));
    k.lo = lo, k.hi = hi, k.use_range = use_range != 0, k.nthres = nthres;
    for (int t = 0; t < nthres; ++t) k.thres[t] = thres[t];
    k.rel = rel;
    Partial* ws = static_cast<Partial*>(workspace);
    hipLaunchKernelGGL(metrics_partial_kernel, dim3(k.tiles, B), dim3(kThreads), 0, s, k, ws);
    if (int rc = check_launch("disp_metrics (partial)")) return rc;
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(kThreads), 0, s, ws, B, k.tiles, H * W, nthres, records,
                       values, batch);
    return check_launch("disp_metrics (final)");
}

int launch_error_map(const float* est, long long eb, long long eh, const float* gt, long long gb, long long gh,
                     float* out, int B, int H, int W, float abs_thres, float rel_thres, hipStream_t s) {
    if (!size_ok(B, H, W)) return arg_error("disp_error_map: sizes must be positive and H * W below 2^31");
    if (!est || !gt || !out) return arg_error("disp_error_map: null pointer");
    if (eb < 0 || eh < 0 || gb < 0 || gh < 0) return arg_error("disp_error_map: negative stride");
    const long long n = static_cast<long long>(B) * H * W;
    if (n > (1LL << 31) * kThreads - 1) return arg_error("disp_error_map: too many pixels for one launch");
    hipLaunchKernelGGL(error_map_kernel, dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, s, est, eb, eh, gt, gb, gh,
                       out, H, W, abs_thres, rel_thres, n);
    return check_launch("disp_error_map");
}

}  // namespace esm

extern "C" {

long long esm_disp_metrics_workspace(int B, int H, int W) { return esm::metrics_workspace(B, H, W); }

int esm_disp_metrics_f32(const float* est, int64_t est_sb, int64_t est_sh, const float* gt, int64_t gt_sb,
                         int64_t gt_sh, const uint8_t* mask, int64_t mask_sb, int64_t mask_sh, int B, int H, int W,
                         float lo, float hi, int use_range, const float* thres, int nthres, float rel,
                         void* workspace, double* records, float* values, float* batch, void* stream) {
    return esm::launch_metrics(est, est_sb, est_sh, gt, gt_sb, gt_sh, mask, mask_sb, mask_sh, B, H, W, lo, hi,
                               use_range, thres, nthres, rel, workspace, records, values, batch,
                               esm::as_stream(stream));
}

int esm_disp_error_map_f32(const float* est, int64_t est_sb, int64_t est_sh, const float* gt, int64_t gt_sb,
                           int64_t gt_sh, float* out, int B, int H, int W, float abs_thres, float rel_thres,
                           void* stream) {
    return esm::launch_error_map(est, est_sb, est_sh, gt, gt_sb, gt_sh, out, B, H, W, abs_thres, rel_thres,
                                 esm::as_stream(stream));
}

}  // extern "C"
