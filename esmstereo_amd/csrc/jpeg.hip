// Baseline JPEG (JFIF) encoding on the device: the entropy-coded scan of an 8-bit colour frame.
//
// The last per-frame host step of the four reference nodes is the MJPG video writer (kitti_publisher_cuda_node.cpp:
// 122-132, kitti_publisher_conf_cuda_node.cpp:265-275, virtual_kitti_publisher_cuda_node.cpp:218-228,
// kitti_publisher_ess_cuda_node.cpp:227-237: cv::VideoWriter with fourcc('M','J','P','G') and
// video_writer.write(combined)), which downloads the stacked picture raw and compresses it on one core.  The picture is already on the device
// (node.dev_frame), so the scan is built here.  The arithmetic is this library's own definition, stated in
// include/esmstereo_amd.h (colour, 4:2:0 averaging, the integer DCT, quantisation, the Annex K.3 Huffman tables,
// restart markers); tests/jpeg_ref.py restates it in numpy and the device bytes equal it byte for byte.
//
// JPEG's Huffman tables are fixed and a restart marker ends on a byte boundary with the DC predictors reset, so
// every restart interval (Ri <= 16 MCUs) is an independent byte string: one workgroup of 256 encodes one interval.
// Three stream-ordered launches per call, the whole batch in each, no host synchronisation and no allocation:
//   1 jpeg_interval_kernel<.., false>  one workgroup per interval: pixels (edge-replicated) -> Y Cb Cr samples in
//                        LDS, the row and column DCT passes, quantisation into zigzag order, then per 8x8 block one
//                        wave with a lane per zigzag position: __ballot gives the non-zero mask, a lane's run is the
//                        distance to the set bit below it, a wave prefix sum of the code lengths gives its bit offset;
//                        the bits are ORed MSB-first into a staging buffer the workgroup zeroed itself, padded with
//                        1-bits, and the 0xFF bytes are counted.  Stores the interval's stuffed length + 2 (the
//                        marker).
//   2 jpeg_scan_kernel   one workgroup per image: the lengths scanned into 64-bit byte offsets; lengths[b].
//   3 jpeg_interval_kernel<.., true>   the same work again (as png.hip's emit launch recomputes its filter), then each
//                        lane stores its run of staged bytes, a 0x00 behind every 0xFF, at the interval's offset, and
//                        lane 0 the marker (RSTn, or EOI behind the last interval).
// Launch 3 recomputes instead of copying a parked segment: parking needs a workspace of the worst case per interval
// (20 KB at Ri = 8, 9 MB for a 750 x 1242 frame) against 12 bytes per interval here.  Only this form was built and
// measured.
// Output stores are single bytes at disjoint positions (no interval shares a byte with another, so nothing depends on
// the order of workgroups and nothing needs zeroing first), each compared with the image's slot in store_slot.
// Staging indices pass through LDS (the block offsets), so put_bits compares the dword index with the staging size.
//
// LDS per workgroup, sized for Ri = 16: 4:2:0 (96 blocks) 6,144 B samples + 12,288 B row pass + 12,288 B quantised
// + 19,904 B staging (a block is at most 20 + 63 * 26 = 1,658 bits: a 9-bit DC code with 11 value bits, then 63 times
// a 16-bit AC code with 10 value bits; ZRL spends 11 bits on 16 coefficients) + 3,376 B tables and offsets = 54,000 B:
// two workgroups (8 waves) per CU of 163,840 B for certain, three only if the allocation granule leaves 3 x 54,000 =
// 162,000 B room (not measured).  4:4:4 (48 blocks) 28,500 B: five workgroups per CU.
#include <climits>
#include <initializer_list>

#include "common.h"
#include "scan.h"

namespace esm {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxRi = 16;
constexpr int kBlockBits = 20 + 63 * 26;  // 1658
constexpr int kHeaderBytes = 629;

struct JpegTables {
    uint8_t base[2][64];     // Annex K.1, K.2, natural order
    uint8_t zigzag[64];      // zigzag position -> natural index
    uint8_t izigzag[64];     // natural index -> zigzag position
    uint8_t dc_bits[2][16], ac_bits[2][16];
    uint8_t dc_vals[2][12], ac_vals[2][162];
    uint32_t dc[2][12];      // code | length << 16, by size
    uint32_t ac[2][256];     // by run << 4 | size
    int16_t m[64];           // round(8192 * 1/2 C(k) cos((2n + 1) k pi / 16)), [k][n]
};

constexpr void huff_lut(const uint8_t* bits, const uint8_t* vals, uint32_t* lut) {
    uint32_t code = 0;
    int i = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int n = 0; n < bits[len - 1]; ++n) lut[vals[i++]] = code++ | static_cast<uint32_t>(len) << 16;
        code <<= 1;
    }
}

constexpr JpegTables make_tables() {
    JpegTables t{};
    constexpr uint8_t base[2][64] = {
        {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
         69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
         81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
        {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
    constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    constexpr uint8_t dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                        {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    constexpr uint8_t ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    constexpr uint8_t ac_vals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
         0x14, 0x32, 0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72,
         0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37,
         0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
         0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
         0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
         0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
         0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
         0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1,
         0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36,
         0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
         0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A,
         0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A,
         0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
         0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
         0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}};
    constexpr int16_t m[64] = {2896, 2896,  2896,  2896,  2896,  2896,  2896,  2896,   //
                               4017, 3406,  2276,  799,   -799,  -2276, -3406, -4017,  //
                               3784, 1567,  -1567, -3784, -3784, -1567, 1567,  3784,   //
                               3406, -799,  -4017, -2276, 2276,  4017,  799,   -3406,  //
                               2896, -2896, -2896, 2896,  2896,  -2896, -2896, 2896,   //
                               2276, -4017, 799,   3406,  -3406, -799,  4017,  -2276,  //
                               1567, -3784, 3784,  -1567, -1567, 3784,  -3784, 1567,   //
                               799,  -2276, 3406,  -4017, 4017,  -3406, 2276,  -799};
    for (int c = 0; c < 2; ++c) {
        for (int i = 0; i < 64; ++i) t.base[c][i] = base[c][i];
        for (int i = 0; i < 16; ++i) {
            t.dc_bits[c][i] = dc_bits[c][i];
            t.ac_bits[c][i] = ac_bits[c][i];
        }
        for (int i = 0; i < 12; ++i) t.dc_vals[c][i] = static_cast<uint8_t>(i);
        for (int i = 0; i < 162; ++i) t.ac_vals[c][i] = ac_vals[c][i];
        huff_lut(t.dc_bits[c], t.dc_vals[c], t.dc[c]);
        huff_lut(t.ac_bits[c], t.ac_vals[c], t.ac[c]);
    }
    for (int i = 0; i < 64; ++i) {
        t.zigzag[i] = zz[i];
        t.izigzag[zz[i]] = static_cast<uint8_t>(i);
        t.m[i] = m[i];
    }
    return t;
}

constexpr JpegTables kHostTables = make_tables();
__constant__ JpegTables kTables = make_tables();

// libjpeg's quality scaling: the percentage applied to the base tables
__host__ __device__ inline int quality_scale(int quality) { return quality < 50 ? 5000 / quality : 200 - 2 * quality; }
__host__ __device__ inline int quant_entry(int base, int scale) {
    const int q = (base * scale + 50) / 100;
    return q < 1 ? 1 : q > 255 ? 255 : q;
}

struct JpegJob {
    const uint8_t* src;
    unsigned long long* offs;  // [B][nint] byte offsets of the intervals in their image's scan
    uint32_t* lens;            // [B][nint] stuffed bytes + 2
    uint8_t* out;              // slots of slot_bytes bytes
    int32_t* lengths;
    long long src_image;       // bytes between images of src
    long long slot_bytes;
    int h, w, bgr, scale, ri;
    int mcu_cols, nmcu;
    uint32_t nint;
};

// the only way into the output: byte `pos` of the image's slot, refused outside it
__device__ __forceinline__ void store_slot(const JpegJob& j, uint8_t* slot, long long pos, uint32_t v) {
    if (pos >= 0 && pos < j.slot_bytes) slot[pos] = static_cast<uint8_t>(v);
}

// n <= 32 bits of val at bit p of the stream, most significant first: bit p is bit 31 - (p & 31) of dword p >> 5
template <int DWORDS>
__device__ __forceinline__ void put_bits(uint32_t* stage, uint32_t p, uint32_t val, uint32_t n) {
    if (n == 0) return;
    const uint32_t i = p >> 5;
    if (i + 1 >= static_cast<uint32_t>(DWORDS)) return;  // (never taken with a sound offset)
    const unsigned long long x = static_cast<unsigned long long>(val) << (64 - (p & 31) - n);
    const uint32_t hi = static_cast<uint32_t>(x >> 32), lo = static_cast<uint32_t>(x);
    if (hi) atomicOr(&stage[i], hi);
    if (lo) atomicOr(&stage[i + 1], lo);
}

struct LaneCode {
    uint32_t bits, len;  // the Huffman code and the value bits behind it, len <= 27
    uint32_t nzrl;       // ZRL codes in front of it, <= 3
};

// ------------------------------------------------------------------------------ 1 and 3: one restart interval
template <bool S420, bool EMIT>
__global__ void __launch_bounds__(kThreads) jpeg_interval_kernel(JpegJob j) {
    constexpr int kBpm = S420 ? 6 : 3;  // blocks per MCU
    constexpr int kBlocks = kMaxRi * kBpm;
    constexpr int kStageDwords = (kBlocks * kBlockBits + 31) / 32 + 2;
    __shared__ uint8_t samp[kBlocks * 64];
    __shared__ int16_t rowp[kBlocks * 64];  // |t| <= (8 * 2896 * 128 + 512) >> 10 = 2896
    __shared__ int16_t quant[kBlocks * 64];  // zigzag order
    __shared__ uint32_t stage[kStageDwords];
    __shared__ uint32_t ac[2][256], dc[2][12];
    __shared__ uint16_t qt[2][64];
    __shared__ int16_t msh[64];
    __shared__ uint8_t izz[64];
    __shared__ uint32_t bbits[kBlocks], boff[kBlocks];
    __shared__ uint32_t wsum[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const uint32_t iv = blockIdx.x;
    const long long b = blockIdx.y;
    const int m0 = static_cast<int>(iv) * j.ri;
    const int nm = min(j.ri, j.nmcu - m0);
    const int nblk = nm * kBpm;

    for (int i = t; i < 512; i += kThreads) (&ac[0][0])[i] = (&kTables.ac[0][0])[i];
    if (t < 24) (&dc[0][0])[t] = (&kTables.dc[0][0])[t];
    if (t < 128) (&qt[0][0])[t] = static_cast<uint16_t>(quant_entry((&kTables.base[0][0])[t], j.scale));
    if (t < 64) {
        msh[t] = kTables.m[t];
        izz[t] = kTables.izigzag[t];
    }
    {
        const int nz = min((nblk * kBlockBits + 31) / 32 + 2, kStageDwords);
        for (int i = t; i < nz; i += kThreads) stage[i] = 0;
    }

    // pixels -> samples; the image is padded to whole MCUs by replicating its last column and row
    const uint8_t* img = j.src + b * j.src_image;
    auto ycc = [&](int gy, int gx, int& y, int& cb, int& cr) {
        const uint8_t* p = img + (static_cast<long long>(min(gy, j.h - 1)) * j.w + min(gx, j.w - 1)) * 3;
        const int c0 = p[0], g = p[1], c2 = p[2];
        const int r = j.bgr ? c2 : c0, bl = j.bgr ? c0 : c2;
        y = (19595 * r + 38470 * g + 7471 * bl + 32768) >> 16;
        cb = (-11059 * r - 21709 * g + 32768 * bl + 8421375) >> 16;
        cr = (32768 * r - 27439 * g - 5329 * bl + 8421375) >> 16;
    };
    if constexpr (S420) {
        const int ly = t >> 4, lx = t & 15;
        for (int m = 0; m < nm; ++m) {
            const int mm = m0 + m, my = mm / j.mcu_cols, mx = mm - my * j.mcu_cols;
            int y, cb, cr;
            ycc(16 * my + ly, 16 * mx + lx, y, cb, cr);
            samp[(m * 6 + (ly >> 3) * 2 + (lx >> 3)) * 64 + (ly & 7) * 8 + (lx & 7)] = static_cast<uint8_t>(y);
            // the 2 x 2 neighbours are lanes ^ 1 and ^ 16 of the same wave (a wave holds four rows of 16)
            cb += __shfl_xor(cb, 1);
            cr += __shfl_xor(cr, 1);
            cb += __shfl_xor(cb, 16);
            cr += __shfl_xor(cr, 16);
            if (((ly | lx) & 1) == 0) {
                const int i = (ly >> 1) * 8 + (lx >> 1);
                samp[(m * 6 + 4) * 64 + i] = static_cast<uint8_t>((cb + 2) >> 2);
                samp[(m * 6 + 5) * 64 + i] = static_cast<uint8_t>((cr + 2) >> 2);
            }
        }
    } else {
        for (int m = wave; m < nm; m += kThreads / 64) {
            const int mm = m0 + m, my = mm / j.mcu_cols, mx = mm - my * j.mcu_cols;
            int y, cb, cr;
            ycc(8 * my + (lane >> 3), 8 * mx + (lane & 7), y, cb, cr);
            samp[(m * 3 + 0) * 64 + lane] = static_cast<uint8_t>(y);
            samp[(m * 3 + 1) * 64 + lane] = static_cast<uint8_t>(cb);
            samp[(m * 3 + 2) * 64 + lane] = static_cast<uint8_t>(cr);
        }
    }
    __syncthreads();

    // rows: t[y][u] = (sum_n M[u][n] (s[y][n] - 128) + 512) >> 10
    for (int idx = t; idx < nblk * 64; idx += kThreads) {
        const int u = idx & 7, row = idx & ~7;
        int sum = 0;
#pragma unroll
        for (int n = 0; n < 8; ++n) sum += msh[u * 8 + n] * (static_cast<int>(samp[row + n]) - 128);
        rowp[idx] = static_cast<int16_t>((sum + 512) >> 10);
    }
    __syncthreads();
    // columns: c8[v][u] = (sum_y M[v][y] t[y][u] + 4096) >> 13, then q = sgn(c8) (|c8| + 4 Q) / (8 Q): an exact
    // integer division
    for (int idx = t; idx < nblk * 64; idx += kThreads) {
        const int k = idx >> 6, vu = idx & 63, v = vu >> 3, u = vu & 7;
        int sum = 0;
#pragma unroll
        for (int y = 0; y < 8; ++y) sum += msh[v * 8 + y] * rowp[k * 64 + y * 8 + u];
        const int c8 = (sum + 4096) >> 13;
        const int jb = k % kBpm;
        const uint32_t q = qt[S420 ? jb >= 4 : jb >= 1][vu];
        uint32_t a = (static_cast<uint32_t>(abs(c8)) + 4 * q) / (8 * q);
        if (vu) a = min(a, 1023u);
        quant[k * 64 + izz[vu]] = static_cast<int16_t>(c8 < 0 ? -static_cast<int>(a) : static_cast<int>(a));
    }
    __syncthreads();

    // a lane's code for zigzag position `lane` of block k (the whole wave calls it)
    const uint32_t zrl_luma = ac[0][0xF0], zrl_chroma = ac[1][0xF0];
    auto code_of = [&](int k) {
        const int jb = k % kBpm;
        const int chroma = S420 ? jb >= 4 : jb >= 1;
        int v = quant[k * 64 + lane];
        if (lane == 0) {  // the difference from the previous block of the same component in this interval
            const int prev = S420 ? (jb == 0 ? k - 3 : jb < 4 ? k - 1 : k - 6) : k - 3;
            if (prev >= 0) v -= quant[prev * 64];
        }
        const unsigned long long nzmask = __ballot(lane == 0 || v != 0);
        const uint32_t a = static_cast<uint32_t>(abs(v));
        const uint32_t size = a ? 32 - __clz(a) : 0;
        const uint32_t vbits = static_cast<uint32_t>(v >= 0 ? v : v + (1 << size) - 1);
        LaneCode c{0, 0, 0};
        uint32_t e = 0;
        if (lane == 0) {
            e = dc[chroma][min(size, 11u)];
        } else if (v != 0) {
            const unsigned long long below = nzmask & ((1ull << lane) - 1);  // bit 0 is always set
            const uint32_t run = lane - (63 - __clzll(below)) - 1;
            c.nzrl = run >> 4;
            e = ac[chroma][(run & 15) << 4 | min(size, 10u)];
        } else if (lane == 63) {
            e = ac[chroma][0];  // end of block
        }
        if (e) {
            c.bits = (e & 0xFFFF) << size | vbits;
            c.len = (e >> 16) + size;
        }
        return c;
    };
    for (int k = wave; k < nblk; k += kThreads / 64) {
        const LaneCode c = code_of(k);
        const uint32_t z = (S420 ? k % kBpm >= 4 : k % kBpm >= 1) ? zrl_chroma : zrl_luma;
        const uint32_t bits = wave_sum(c.len + c.nzrl * (z >> 16));
        if (lane == 0) bbits[k] = bits;
    }
    __syncthreads();
    if (t < nblk) {
        uint32_t s = 0;
        for (int i = 0; i < t; ++i) s += bbits[i];
        boff[t] = s;
    }
    __syncthreads();
    const uint32_t total_bits = boff[nblk - 1] + bbits[nblk - 1];
    for (int k = wave; k < nblk; k += kThreads / 64) {
        const LaneCode c = code_of(k);
        const uint32_t z = (S420 ? k % kBpm >= 4 : k % kBpm >= 1) ? zrl_chroma : zrl_luma;
        const uint32_t zl = z >> 16, zc = z & 0xFFFF;
        const uint32_t mine = c.len + c.nzrl * zl;
        uint32_t pos = boff[k] + wave_inclusive(mine) - mine;
        for (uint32_t i = 0; i < c.nzrl; ++i, pos += zl) put_bits<kStageDwords>(stage, pos, zc, zl);
        put_bits<kStageDwords>(stage, pos, c.bits, c.len);
    }
    if (t == 0) {  // pad the last byte with 1-bits
        const uint32_t pad = (8 - (total_bits & 7)) & 7;
        put_bits<kStageDwords>(stage, total_bits, (1u << pad) - 1, pad);
    }
    __syncthreads();

    // byte stuffing: each lane owns a run of `per` staged dwords; a prefix sum over "byte == 0xFF" places it
    const uint32_t nbytes = (total_bits + 7) >> 3;
    const uint32_t ndw = (nbytes + 3) >> 2;
    const uint32_t per = (ndw + kThreads - 1) / kThreads;
    const uint32_t d0 = min(t * per, ndw), d1 = min(d0 + per, ndw);
    uint32_t ff = 0;
    for (uint32_t d = d0; d < d1; ++d) {
        const uint32_t word = stage[d];
#pragma unroll
        for (int k = 0; k < 4; ++k) ff += 4 * d + k < nbytes && ((word >> (24 - 8 * k)) & 0xFF) == 0xFF;
    }
    uint32_t total_ff;
    const uint32_t ff_before = block_scan<kThreads>(ff, wsum, total_ff);
    const long long at = b * static_cast<long long>(j.nint) + iv;
    if constexpr (!EMIT) {
        if (t == 0) j.lens[at] = nbytes + total_ff + 2;
    } else {
        uint8_t* slot = j.out + b * j.slot_bytes;
        const long long base = static_cast<long long>(j.offs[at]);
        long long pos = base + 4LL * d0 + ff_before;
        for (uint32_t d = d0; d < d1; ++d) {
            const uint32_t word = stage[d];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t byte = (word >> (24 - 8 * k)) & 0xFF;
                if (4 * d + k < nbytes) {
                    store_slot(j, slot, pos++, byte);
                    if (byte == 0xFF) store_slot(j, slot, pos++, 0);
                }
            }
        }
        if (t == 0) {  // RSTn in front of the next interval, EOI behind the last
            const long long end = base + nbytes + total_ff;
            store_slot(j, slot, end, 0xFF);
            store_slot(j, slot, end + 1, iv + 1 == j.nint ? 0xD9 : 0xD0 + (iv & 7));
        }
    }
}

// -------------------------------------------------------------------------------------------- 2: offsets, length
__global__ void __launch_bounds__(kThreads) jpeg_scan_kernel(JpegJob j) {
    __shared__ uint32_t wsum[kThreads / 64];
    const long long b = blockIdx.x;
    const uint32_t* lens = j.lens + b * static_cast<long long>(j.nint);
    unsigned long long* offs = j.offs + b * static_cast<long long>(j.nint);
    unsigned long long carry = 0;
    for (uint32_t c0 = 0; c0 < j.nint; c0 += kThreads) {
        const uint32_t c = c0 + threadIdx.x;
        const uint32_t len = c < j.nint ? lens[c] : 0;  // <= 2 * 19,896 + 2 each: a round's total fits 32 bits
        uint32_t total;
        const uint32_t off = block_scan<kThreads>(len, wsum, total);
        if (c < j.nint) offs[c] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) {
        int32_t n;
        if (carry > static_cast<unsigned long long>(INT_MAX))
            n = INT_MIN;
        else if (static_cast<long long>(carry) > j.slot_bytes)
            n = -static_cast<int32_t>(carry);
        else
            n = static_cast<int32_t>(carry);
        j.lengths[b] = n;
    }
}

struct Geometry {
    int bpm, mcu_cols, nmcu;
    long long nint;
};

const char* geometry(int h, int w, int subsampling, int restart_mcus, Geometry& g) {
    if (h < 1 || w < 1 || h > 65535 || w > 65535) return "height / width outside 1..65535";
    if (3LL * h * w >= (1LL << 31)) return "3 h w >= 2^31";
    if (subsampling != 420 && subsampling != 444) return "subsampling must be 420 or 444";
    if (restart_mcus < 1 || restart_mcus > kMaxRi) return "restart_mcus outside 1..16";
    const int mcu = subsampling == 420 ? 16 : 8;
    g.bpm = subsampling == 420 ? 6 : 3;
    g.mcu_cols = (w + mcu - 1) / mcu;
    g.nmcu = g.mcu_cols * ((h + mcu - 1) / mcu);  // < 2^25
    g.nint = (g.nmcu + restart_mcus - 1) / restart_mcus;
    return nullptr;
}

// the most bytes an interval of `mcus` MCUs can take with its marker: every staged byte may be 0xFF
long long interval_bound(int mcus, int bpm) {
    return 2 * ((static_cast<long long>(mcus) * bpm * kBlockBits + 7) / 8) + 2;
}

}  // namespace
}  // namespace esm

extern "C" {

int esm_jpeg_quant_table(int quality, int which, uint8_t out64[64]) {
    if (!out64) return esm::arg_error("jpeg_quant_table: null pointer");
    if (quality < 1 || quality > 100) return esm::arg_error("jpeg_quant_table: quality outside 1..100");
    if (which != 0 && which != 1) return esm::arg_error("jpeg_quant_table: which must be 0 (luminance) or 1");
    const int s = esm::quality_scale(quality);
    for (int i = 0; i < 64; ++i) out64[i] = static_cast<uint8_t>(esm::quant_entry(esm::kHostTables.base[which][i], s));
    return ESM_OK;
}

int esm_jpeg_header(uint8_t* buf, int cap, int w, int h, int quality, int subsampling, int restart_mcus) {
    esm::Geometry g;
    if (!buf) return esm::arg_error("jpeg_header: null pointer");
    if (const char* e = esm::geometry(h, w, subsampling, restart_mcus, g))
        return esm::arg_error(std::string("jpeg_header: ") + e);
    if (quality < 1 || quality > 100) return esm::arg_error("jpeg_header: quality outside 1..100");
    if (cap < esm::kHeaderBytes) return esm::arg_error("jpeg_header: the buffer is smaller than the 629-byte header");
    const esm::JpegTables& T = esm::kHostTables;
    uint8_t* p = buf;
    auto put = [&](std::initializer_list<int> bytes) {
        for (int v : bytes) *p++ = static_cast<uint8_t>(v);
    };
    put({0xFF, 0xD8});
    put({0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    const int s = esm::quality_scale(quality);
    for (int c = 0; c < 2; ++c) {
        put({0xFF, 0xDB, 0x00, 0x43, c});
        for (int i = 0; i < 64; ++i) *p++ = static_cast<uint8_t>(esm::quant_entry(T.base[c][T.zigzag[i]], s));
    }
    put({0xFF, 0xC0, 0x00, 0x11, 8, h >> 8, h & 0xFF, w >> 8, w & 0xFF, 3});
    put({1, subsampling == 420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
    for (int id = 0; id < 2; ++id) {
        for (int cls = 0; cls < 2; ++cls) {
            const int n = cls ? 162 : 12;
            put({0xFF, 0xC4, 0x00, 19 + n, cls << 4 | id});
            for (int i = 0; i < 16; ++i) *p++ = cls ? T.ac_bits[id][i] : T.dc_bits[id][i];
            for (int i = 0; i < n; ++i) *p++ = cls ? T.ac_vals[id][i] : T.dc_vals[id][i];
        }
    }
    put({0xFF, 0xDD, 0x00, 0x04, 0x00, restart_mcus});
    put({0xFF, 0xDA, 0x00, 0x0C, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0x00, 0x3F, 0x00});
    return static_cast<int>(p - buf);
}

long long esm_jpeg_stream_bound(int h, int w, int subsampling, int restart_mcus) {
    esm::Geometry g;
    if (const char* e = esm::geometry(h, w, subsampling, restart_mcus, g))
        return esm::arg_error(std::string("jpeg_stream_bound: ") + e);
    const int tail = g.nmcu - static_cast<int>(g.nint - 1) * restart_mcus;
    return (g.nint - 1) * esm::interval_bound(restart_mcus, g.bpm) + esm::interval_bound(tail, g.bpm);
}

long long esm_jpeg_workspace_bytes(int B, int h, int w, int subsampling, int restart_mcus) {
    esm::Geometry g;
    if (B < 1 || B > 65535) return esm::arg_error("jpeg_workspace_bytes: B outside 1..65535");
    if (const char* e = esm::geometry(h, w, subsampling, restart_mcus, g))
        return esm::arg_error(std::string("jpeg_workspace_bytes: ") + e);
    return 12LL * B * g.nint;
}

int esm_jpeg_encode_rgb8(const uint8_t* src, int B, int h, int w, int bgr, int quality, int subsampling,
                         int restart_mcus, void* work, uint8_t* out, long long slot_bytes, int32_t* lengths,
                         void* stream) {
    esm::Geometry g;
    if (!src || !work || !out || !lengths) return esm::arg_error("jpeg_encode_rgb8: null pointer");
    if (B < 1 || B > 65535) return esm::arg_error("jpeg_encode_rgb8: B outside 1..65535");
    if (const char* e = esm::geometry(h, w, subsampling, restart_mcus, g))
        return esm::arg_error(std::string("jpeg_encode_rgb8: ") + e);
    if (quality < 1 || quality > 100) return esm::arg_error("jpeg_encode_rgb8: quality outside 1..100");
    if (slot_bytes < 2) return esm::arg_error("jpeg_encode_rgb8: a slot below 2 bytes");
    if (reinterpret_cast<uintptr_t>(work) % 8) return esm::arg_error("jpeg_encode_rgb8: work not 8-byte aligned");
    esm::JpegJob j{};
    j.src = src;
    j.offs = static_cast<unsigned long long*>(work);
    j.lens = reinterpret_cast<uint32_t*>(j.offs + static_cast<long long>(B) * g.nint);
    j.out = out;
    j.lengths = lengths;
    j.src_image = 3LL * h * w;
    j.slot_bytes = slot_bytes;
    j.h = h;
    j.w = w;
    j.bgr = bgr != 0;
    j.scale = esm::quality_scale(quality);
    j.ri = restart_mcus;
    j.mcu_cols = g.mcu_cols;
    j.nmcu = g.nmcu;
    j.nint = static_cast<uint32_t>(g.nint);
    hipStream_t s = esm::as_stream(stream);
    const dim3 grid(j.nint, B), block(esm::kThreads);
    if (subsampling == 420) {
        hipLaunchKernelGGL((esm::jpeg_interval_kernel<true, false>), grid, block, 0, s, j);
        hipLaunchKernelGGL(esm::jpeg_scan_kernel, dim3(B), block, 0, s, j);
        hipLaunchKernelGGL((esm::jpeg_interval_kernel<true, true>), grid, block, 0, s, j);
    } else {
        hipLaunchKernelGGL((esm::jpeg_interval_kernel<false, false>), grid, block, 0, s, j);
        hipLaunchKernelGGL(esm::jpeg_scan_kernel, dim3(B), block, 0, s, j);
        hipLaunchKernelGGL((esm::jpeg_interval_kernel<false, true>), grid, block, 0, s, j);
    }
    return esm::check_launch("jpeg_encode_rgb8");
}

}  // extern "C"
