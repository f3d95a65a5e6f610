// Probe: does a lean conv start sooner when the addresses of its first loads come from kernel arguments that
// gfx950 preloads into SGPRs at wave launch (LLVM -amdgpu-kernarg-preload-count), instead of from the s_load of
// the by-value esm_conv_desc?  
//
// One small kernel shaped like the tap-plane split of conv_small.hip: a 16-wave workgroup finishes one
// 16-cout x 16-pixel tile of a 16 -> 16 channel conv with 4 x 3 x 3 taps (4 channel groups x 4 tap planes = one
// unit of 9 taps per wave): 9 + 9 dependent-address buffer_loads and 2 BN constants, 9 MFMAs, the partial tiles
// summed through LDS in wave order, one store per lane of the first four waves.  Each launch reads the one
// before it; 32 launches are captured into a graph and replayed between one event pair.
//
// Variants (argv[1]):
//   A  every argument in one by-value esm_conv_desc (what the library's kernels do)
//   B  the first loads' addresses from 14 leading scalar dwords, the descriptor behind them (output side only);
//      BN constants [scale | shift] behind the packed weights, read through the weight descriptor
//   C  B's kernel in a binary compiled with -mllvm -amdgpu-kernarg-preload-count=14
//   D  as B, but the BN constants keep their own pointers: two more arguments between the 14 dwords and the
//      descriptor (the weights' packing stays as it is)
//   E  D's kernel in the binary compiled with the option
// B / C and D / E are the same source: which one a binary holds is decided by how it was compiled, so the driver
// (scripts/gpu_kernarg_probe.sh) builds two binaries and runs A, B, D from the first and C, E from the second.
//
// Output, one line per grid: variant, workgroups, us per launch, FNV-1a hash of the final tensor (the driver
// checks that every variant's hash agrees).
//
// Build: hipcc -O3 --offload-arch=gfx950 -I include [-mllvm -amdgpu-kernarg-preload-count=14] -o probe this.hip
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "esmstereo_amd.h"

#define CK(x)                                                                              \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, hipGetErrorString(e_));     \
            return 1;                                                                      \
        }                                                                                  \
    } while (0)

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr unsigned kOOB = 0x40000000u;  // offset marker past the end of every buffer (spans < 1 GiB)
constexpr int kC = 16;                  // channels in and out
constexpr int kTaps = 36;               // 4 x 3 x 3
constexpr int kWaves = 16;
constexpr int kChain = 32;

__device__ __forceinline__ int fast_div(int n, unsigned m) {
    return m ? static_cast<int>(__umulhi(static_cast<unsigned>(n), m)) : n;
}
static unsigned magic_for(int d) {
    return d <= 1 ? 0u : static_cast<unsigned>(((1ull << 32) + static_cast<unsigned long long>(d) - 1) / d);
}

// what a wave needs to issue its first batch of loads
struct First {
    const float* src;
    const float* w;
    int sb, sc, sd, sh;
    unsigned m_ds, m_b;
    int Wi, Hi, Di, B, Cin, Cout, cout_pad, pd, ph, pw;
    const float* scale;  // BN constants: own pointers, or null = behind the packed weights
    const float* shift;
};

template <bool BNW>
__device__ __forceinline__ void body(const First& f, const esm_conv_desc& a) {
    __shared__ __attribute__((aligned(16))) float red[kWaves * 4 * 64];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n16 = lane & 15, kq = lane >> 4;

    const int x0 = blockIdx.x * 16, ys = blockIdx.y, zz = blockIdx.z;
    const int r1 = fast_div(zz, f.m_ds);
    const int zs = zz - r1 * f.Di;
    const int r2 = fast_div(r1, f.m_b);
    const int b = r1 - r2 * f.B;

    const int wtap = 16 * f.cout_pad;  // cin_pad = 16
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(f.w), static_cast<short>(0), 4 * (kTaps * wtap + 2 * f.cout_pad), 0x00020000);

    // epilogue constants of the element this thread finishes, loaded up front
    const int ej = (tid >> 6) & 3;
    const int co = min(4 * kq + ej, f.Cout - 1);
    float scl, shf;
    if constexpr (BNW) {
        scl = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, 4 * co, 4 * kTaps * wtap, 0));
        shf = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(wrs, 4 * (f.cout_pad + co), 4 * kTaps * wtap, 0));
    } else {
        scl = f.scale[co];
        shf = f.shift[co];
    }

    const int xs = x0 + n16;
    unsigned xoff[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int xi = xs - f.pw + t;
        xoff[t] = (xs < f.Wi && xi >= 0 && xi < f.Wi) ? 4u * xi : kOOB;
    }
    const int g = wave >> 2, dz = wave & 3, c0 = 4 * g;
    const int zi = zs - f.pd + dz;
    const bool zok = zi >= 0 && zi < f.Di;

    const int span = 4 * ((f.Cin - 1) * f.sc + (f.Di - 1) * f.sd + (f.Hi - 1) * f.sh + f.Wi);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(f.src + static_cast<long long>(b) * f.sb), static_cast<short>(0), span, 0x00020000);
    const unsigned chv = (c0 + kq < f.Cin) ? 4u * (c0 + kq) * f.sc : kOOB;
    const unsigned wl = 4u * (kq * f.cout_pad + n16);

    float bv[9], av[9];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yi = ys - f.ph + dy;
        const int roff = (zok && yi >= 0 && yi < f.Hi) ? 4 * (zi * f.sd + yi * f.sh) : static_cast<int>(kOOB);
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int t = dy * 3 + dx;
            bv[t] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, static_cast<int>(chv + xoff[dx]), roff, 0));
            av[t] = __uint_as_float(
                __builtin_amdgcn_raw_buffer_load_b32(wrs, static_cast<int>(wl), 4 * ((dz * 9 + t) * wtap + c0 * f.cout_pad), 0));
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    floatx4 acc[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[t], bv[t], acc[t & 1], 0, 0, 0);

#pragma unroll
    for (int j = 0; j < 4; ++j) red[(wave * 4 + j) * 64 + lane] = acc[0][j] + acc[1][j];
    __syncthreads();
    if (tid >= 256) return;
    float v = red[ej * 64 + lane];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v = v + red[w * 256 + ej * 64 + lane];
    v = fminf(fmaxf(v * scl + shf, -1.f), 1.f);

    // output side: from the descriptor in every variant
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(
        a.out + b * a.ob, static_cast<short>(0),
        4 * ((a.Cout - 1) * static_cast<int>(a.oc) + (a.Do - 1) * static_cast<int>(a.od) +
             (a.Ho - 1) * static_cast<int>(a.oh) + a.Wo),
        0x00020000);
    const int orow = 4 * (zs * static_cast<int>(a.od) + ys * static_cast<int>(a.oh));
    const int cw = 4 * kq + ej;
    const unsigned vo = (cw < a.Cout && xs < a.Wo) ? 4u * (cw * static_cast<int>(a.oc) + xs) : kOOB;
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), ro, static_cast<int>(vo), orow, 0);
}

__global__ void __launch_bounds__(64 * kWaves) struct_kernel(const esm_conv_desc a, unsigned m_ds, unsigned m_b) {
    First f;
    f.src = a.src[0].ptr;
    f.w = a.w;
    f.sb = static_cast<int>(a.src[0].sb);
    f.sc = static_cast<int>(a.src[0].sc);
    f.sd = static_cast<int>(a.src[0].sd);
    f.sh = static_cast<int>(a.src[0].sh);
    f.m_ds = m_ds;
    f.m_b = m_b;
    f.Wi = a.Wi, f.Hi = a.Hi, f.Di = a.Di, f.B = a.B, f.Cin = a.Cin, f.Cout = a.Cout, f.cout_pad = a.cout_pad;
    f.pd = a.pd, f.ph = a.ph, f.pw = a.pw;
    f.scale = a.scale;
    f.shift = a.shift;
    body<false>(f, a);
}

// 14 leading scalar dwords: 2 + 2 of pointers, 4 strides, 2 reciprocals, Wi|Hi, Di|Ws, Ds|B, Cin|Cout|cout_pad|pads
__device__ __forceinline__ First unpack(const float* src, const float* w, int sb, int sc, int sd, int sh, unsigned m_ds,
                                        unsigned m_b, unsigned wh, unsigned dw, unsigned db, unsigned cp,
                                        const float* scale, const float* shift) {
    First f;
    f.src = src;
    f.w = w;
    f.sb = sb, f.sc = sc, f.sd = sd, f.sh = sh;
    f.m_ds = m_ds;
    f.m_b = m_b;
    f.Wi = wh & 0xffff, f.Hi = wh >> 16, f.Di = dw & 0xffff, f.B = db >> 16;
    f.Cin = cp & 0xff, f.Cout = (cp >> 8) & 0xff, f.cout_pad = (cp >> 16) & 0x3f;
    f.pd = (cp >> 22) & 0x7, f.ph = (cp >> 25) & 0x7, f.pw = (cp >> 28) & 0x7;
    f.scale = scale;
    f.shift = shift;
    return f;
}

__global__ void __launch_bounds__(64 * kWaves)
    record_kernel(const float* src, const float* w, int sb, int sc, int sd, int sh, unsigned m_ds, unsigned m_b,
                  unsigned wh, unsigned dw, unsigned db, unsigned cp, const esm_conv_desc a) {
    body<true>(unpack(src, w, sb, sc, sd, sh, m_ds, m_b, wh, dw, db, cp, nullptr, nullptr), a);
}

__global__ void __launch_bounds__(64 * kWaves)
    record_bn_kernel(const float* src, const float* w, int sb, int sc, int sd, int sh, unsigned m_ds, unsigned m_b,
                     unsigned wh, unsigned dw, unsigned db, unsigned cp, const float* scale, const float* shift,
                     const esm_conv_desc a) {
    body<false>(unpack(src, w, sb, sc, sd, sh, m_ds, m_b, wh, dw, db, cp, scale, shift), a);
}

static uint64_t fnv1a(const void* p, size_t n) {
    const unsigned char* c = static_cast<const unsigned char*>(p);
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}

static int run(char variant, int D, int H, int W, int replays) {
    const size_t n = static_cast<size_t>(kC) * D * H * W;
    const size_t nw = static_cast<size_t>(kTaps) * 16 * 16 + 32;
    std::vector<float> hx(n), hw(nw);
    uint32_t s = 12345u;
    auto rnd = [&] {
        s = s * 1664525u + 1013904223u;
        return static_cast<float>(s >> 8) * (1.0f / 8388608.0f) - 1.0f;  // [-1, 1)
    };
    for (auto& v : hx) v = rnd();
    for (size_t i = 0; i < nw - 32; ++i) hw[i] = rnd() * (1.0f / 12.0f);
    for (int i = 0; i < 16; ++i) hw[nw - 32 + i] = 1.0f + 0.25f * rnd();
    for (int i = 0; i < 16; ++i) hw[nw - 16 + i] = 0.1f * rnd();

    float *buf[2], *dw;
    CK(hipMalloc(&buf[0], n * 4));
    CK(hipMalloc(&buf[1], n * 4));
    CK(hipMalloc(&dw, nw * 4));
    CK(hipMemcpy(buf[0], hx.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemset(buf[1], 0, n * 4));
    CK(hipMemcpy(dw, hw.data(), nw * 4, hipMemcpyHostToDevice));

    const dim3 grid((W + 15) / 16, H, D);
    const unsigned mds = magic_for(D), mb = magic_for(1);
    hipStream_t st;
    CK(hipStreamCreate(&st));
    hipGraph_t graph;
    hipGraphExec_t exec;
    CK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < kChain; ++i) {
        esm_conv_desc a;
        memset(&a, 0, sizeof a);
        a.src[0].ptr = buf[i & 1];
        a.src[0].C = kC;
        a.src[0].sb = static_cast<int64_t>(n), a.src[0].sc = static_cast<int64_t>(D) * H * W;
        a.src[0].sd = static_cast<int64_t>(H) * W, a.src[0].sh = W;
        a.nsrc = 1, a.B = 1, a.Cin = kC, a.Cout = kC, a.cin_pad = 16, a.cout_pad = 16;
        a.Di = a.Do = D, a.Hi = a.Ho = H, a.Wi = a.Wo = W;
        a.kd = 4, a.kh = a.kw = 3, a.stride = 1, a.pd = a.ph = a.pw = 1;
        a.w = dw, a.scale = dw + nw - 32, a.shift = dw + nw - 16;
        a.out = buf[(i + 1) & 1];
        a.ob = a.src[0].sb, a.oc = a.src[0].sc, a.od = a.src[0].sd, a.oh = W;
        a.post_scale = 1.f;
        const int sb = static_cast<int>(a.src[0].sb), sc = static_cast<int>(a.src[0].sc);
        const int sd = static_cast<int>(a.src[0].sd), sh = static_cast<int>(a.src[0].sh);
        const unsigned wh = W | H << 16, dws = D | W << 16, db = D | 1 << 16;
        const unsigned cp = kC | kC << 8 | 16 << 16 | 1 << 22 | 1 << 25 | 1 << 28;
        if (variant == 'A')
            hipLaunchKernelGGL(struct_kernel, grid, dim3(64 * kWaves), 0, st, a, mds, mb);
        else if (variant == 'B' || variant == 'C')
            hipLaunchKernelGGL(record_kernel, grid, dim3(64 * kWaves), 0, st, a.src[0].ptr, a.w, sb, sc, sd, sh, mds, mb,
                               wh, dws, db, cp, a);
        else
            hipLaunchKernelGGL(record_bn_kernel, grid, dim3(64 * kWaves), 0, st, a.src[0].ptr, a.w, sb, sc, sd, sh, mds,
                               mb, wh, dws, db, cp, a.scale, a.shift, a);
    }
    CK(hipStreamEndCapture(st, &graph));
    CK(hipGetLastError());
    CK(hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0));

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    for (int i = 0; i < 20; ++i) CK(hipGraphLaunch(exec, st));
    CK(hipStreamSynchronize(st));
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < replays; ++i) CK(hipGraphLaunch(exec, st));
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipMemcpy(hx.data(), buf[0], n * 4, hipMemcpyDeviceToHost));
    float amax = 0.f;
    for (float v : hx) amax = v != v ? 1e30f : (v < 0 ? (-v > amax ? -v : amax) : (v > amax ? v : amax));
    printf("%c wgs %5u us_per_launch %7.3f hash %016llx absmax %.4f\n", variant, grid.x * grid.y * grid.z,
           ms * 1e3 / (static_cast<double>(replays) * kChain), static_cast<unsigned long long>(fnv1a(hx.data(), n * 4)), amax);
    CK(hipGraphExecDestroy(exec));
    CK(hipGraphDestroy(graph));
    CK(hipFree(buf[0]));
    CK(hipFree(buf[1]));
    CK(hipFree(dw));
    CK(hipStreamDestroy(st));
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2 || !strchr("ABCDE", argv[1][0])) {
        fprintf(stderr, "usage: %s A|B|C|D|E [replays]\n", argv[0]);
        return 2;
    }
    const int replays = argc > 2 ? atoi(argv[2]) : 300;
    if (run(argv[1][0], 4, 8, 32, replays)) return 1;     // 2 x 8 x 4 = 64 workgroups
    return run(argv[1][0], 12, 24, 78, replays);          // 5 x 24 x 12 = 1440 workgroups (the S-K `agg` grid)
}
