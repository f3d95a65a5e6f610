// PNG encoding on the device: the zlib stream of a 16-bit grayscale map or an 8-bit colour frame, Huffman-only.
//
// The last host step of the save_disp.py flow (save_disp.py:83-88, test_kitti.py:127-131) is the PNG writer:
// io.write_png_u16 / render.write_png_bgr8 download the raw map and run zlib's LZ77 on one core.  For a smooth
// disparity the PNG Sub filter plus an order-0 Huffman code is both smaller and parallel, so the stream is built here:
//
//   78 01                                    zlib header (RFC 1950: deflate, 32 KiB window, no dictionary, level 0 hint)
//   one deflate block, BFINAL = 1, BTYPE = 2 (RFC 1951 section 3.2.7), literals only:
//     HLIT = 0 (257 codes), HDIST = 0 (one distance code of length 1, never used), HCLEN = 15;
//     the code-length alphabet is the fixed complete code "symbols 0-15: 4 bits, 16-18: unused", so each of the 258
//     lengths is one 4-bit code and the block header is always 1106 bits;
//     the image's own canonical code (section 3.2.2), bit-reversed into the LSB-first stream, over the filtered
//     scanlines, then end-of-block
//   pad to a byte, Adler-32 of the filtered scanlines (big-endian)
//
// Filtered scanlines (PNG section 9): per row one filter-type byte, then the row; 16-bit samples big-endian, colour
// as R, G, B.  The filter is one per call: 0 None, 1 Sub (bpp 2 / 3), 2 Up.
//
// Three stream-ordered launches per call, the whole batch in each, no host sync in between.  The raw bytes of an
// image are cut into chunks of kChunk = 3840 bytes: 256 lanes x 15 consecutive bytes.
//   1 png_count_kernel   one workgroup per chunk: the filtered bytes straight from the source (Sub and Up read the
//                        source, so chunks need no hand-off), a 256-bin histogram in LDS, the chunk's Adler partials
//                        (sum d, sum (n - i) d).  Plain stores to the workspace, no global atomics.
//   2 png_table_kernel   one workgroup per image: total histogram + end-of-block, rank sort of the counts across
//                        the workgroup, deflate_lengths_sorted on lane 0, canonical codes, each chunk's bit count
//                        sum hist * len scanned into bit offsets, Adler-32 in 64-bit / reduced arithmetic, the
//                        header, the length, the trailer.  It also zeroes every dword launch 3 will OR into.
//   3 png_emit_kernel    one workgroup per chunk: the filtered bytes again, 15 symbols per lane as four words of at
//                        most 60 bits, a workgroup scan of the lanes' bit counts, OR into an LDS staging buffer the
//                        workgroup zeroed itself, interior dwords out with plain coalesced stores; the at most two
//                        dwords shared with the neighbours by integer atomic OR (order-independent: the bytes are the
//                        same from run to run).
// Every store into the output goes through store_slot / or_slot, which compare the dword index with the slot: an
// offset that is wrong for whatever reason cannot leave the image's slot.  The offsets themselves pass through LDS
// (the scan's wave sums) and the workspace; the staging index is compared with the staging size too.
// The chunk size: staging is 1,808 dwords + a 257-entry table, 8.3 KB per workgroup, far inside 80 KB (two
// workgroups per CU); 15 bytes per lane keeps a lane's 15 codes in four 64-bit words (4 x 15 bits) and makes a chunk
// boundary fall anywhere in a row (3840 = 2^8 * 3 * 5 is a multiple of neither 1 + 2w nor 1 + 3w in general).
// The disparity entry applies esm_disp_to_u16's rounding inside launches 1 and 3: the uint16 map never exists in HBM.
#include <algorithm>

#include "common.h"
#include "deflate_lengths.h"
#include "scan.h"

namespace esm {
namespace {

constexpr int kThreads = 256;
constexpr int kSymPerLane = 15;
constexpr int kChunk = kThreads * kSymPerLane;  // 3840
constexpr int kHeaderBits = 1106;
constexpr int kPreBits = 16 + kHeaderBits;      // zlib header + block header: chunk 0 starts at bit 1122
constexpr int kHeaderDwords = (kPreBits + 31) / 32;  // 36
constexpr int kStageDwords = (31 + kChunk * kDeflateMaxLen + kDeflateMaxLen + 31) / 32 + 6;
constexpr long long kMaxRaw = 1LL << 28;
constexpr uint32_t kAdlerMod = 65521;
constexpr int kTableWords = 260, kMetaWords = 4;

enum { SRC_U16 = 0, SRC_RGB8 = 1, SRC_DISP = 2 };

struct PngJob {
    const void* src;
    uint32_t* work;
    uint32_t* out;        // slots of slot_dwords dwords
    int32_t* lengths;
    long long src_image;  // elements between images of src
    long long work_words; // per image
    long long slot_dwords;
    int rows, w, row_raw;  // row_raw = 1 + bpp * w
    int pitch, top, left;  // SRC_DISP: the padded map's row pitch and the window
    int bgr, filter;
    uint32_t raw, nchunks;
};

// workspace of one image, in 32-bit words: [nchunks][256] histograms, [nchunks][2] Adler partials, [nchunks] bit
// offsets, the code table (code | len << 16), 4 words of totals
__host__ __device__ inline long long work_words(long long nchunks) { return nchunks * 259 + kTableWords + kMetaWords; }
__device__ __forceinline__ uint32_t* ws_hist(const PngJob& j, uint32_t* ws) { return ws; }
__device__ __forceinline__ uint32_t* ws_adler(const PngJob& j, uint32_t* ws) { return ws + 256LL * j.nchunks; }
__device__ __forceinline__ uint32_t* ws_offs(const PngJob& j, uint32_t* ws) { return ws + 258LL * j.nchunks; }
__device__ __forceinline__ uint32_t* ws_table(const PngJob& j, uint32_t* ws) { return ws + 259LL * j.nchunks; }

// one byte of the unfiltered scanline body: row r, byte c of bpp * w
template <int KIND>
__device__ __forceinline__ uint32_t raw_at(const PngJob& j, long long b, int r, int c) {
    if constexpr (KIND == SRC_RGB8) {
        const int px = c / 3, k = c - 3 * px;
        const uint8_t* p = static_cast<const uint8_t*>(j.src) + b * j.src_image;
        return p[(static_cast<long long>(r) * j.w + px) * 3 + (j.bgr ? 2 - k : k)];
    } else {
        uint32_t v;
        if constexpr (KIND == SRC_U16) {
            v = (static_cast<const uint16_t*>(j.src) + b * j.src_image)[static_cast<long long>(r) * j.w + (c >> 1)];
        } else {
            const float* p = static_cast<const float*>(j.src) + b * j.src_image;
            v = disp_u16_value(p[static_cast<long long>(r + j.top) * j.pitch + j.left + (c >> 1)]);
        }
        return (c & 1) ? (v & 0xFF) : (v >> 8);
    }
}

// f(k, d) for the lane's filtered bytes d at chunk-local index 15 * lane + k, k < 15, that exist
template <int KIND, typename F>
__device__ __forceinline__ void for_filtered(const PngJob& j, long long b, uint32_t chunk, F&& f) {
    constexpr int bpp = KIND == SRC_RGB8 ? 3 : 2;
    const uint32_t i0 = chunk * kChunk + threadIdx.x * kSymPerLane;
    if (i0 >= j.raw) return;
    int r = static_cast<int>(i0 / static_cast<uint32_t>(j.row_raw));
    int c = static_cast<int>(i0 - static_cast<uint32_t>(r) * j.row_raw);
    const int n = static_cast<int>(min(static_cast<uint32_t>(kSymPerLane), j.raw - i0));
    static_for<0, kSymPerLane>([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if (k < n) {
            uint32_t d;
            if (c == 0) {
                d = static_cast<uint32_t>(j.filter);
            } else {
                const int x = c - 1;
                d = raw_at<KIND>(j, b, r, x);
                if (j.filter == 1) {
                    if (x >= bpp) d -= raw_at<KIND>(j, b, r, x - bpp);
                } else if (j.filter == 2) {
                    if (r > 0) d -= raw_at<KIND>(j, b, r - 1, x);
                }
                d &= 0xFF;
            }
            f(kc, d);
            if (++c == j.row_raw) {
                c = 0;
                ++r;
            }
        }
    });
}

// the only two ways into the output: dword d of the image's slot, refused outside it
__device__ __forceinline__ void store_slot(const PngJob& j, uint32_t* slot, long long d, uint32_t v) {
    if (d >= 0 && d < j.slot_dwords) slot[d] = v;
}
__device__ __forceinline__ void or_slot(const PngJob& j, uint32_t* slot, long long d, uint32_t v) {
    if (v && d >= 0 && d < j.slot_dwords)
        __hip_atomic_fetch_or(slot + d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------- 1: filter and count
template <int KIND>
__global__ void __launch_bounds__(kThreads) png_count_kernel(PngJob j) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t red[2 * (kThreads / 64)];
    const uint32_t chunk = blockIdx.x;
    const long long b = blockIdx.y;
    uint32_t* ws = j.work + b * j.work_words;
    hist[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = min(static_cast<uint32_t>(kChunk), j.raw - chunk * kChunk);
    uint32_t s1 = 0, s2 = 0;  // sum d <= 3840 * 255, sum (n - i) d <= 255 * 3840 * 3841 / 2 = 1.88e9: both fit 32 bits
    for_filtered<KIND>(j, b, chunk, [&](auto kc, uint32_t d) {
        atomicAdd(&hist[d], 1u);
        s1 += d;
        s2 += (n - (threadIdx.x * kSymPerLane + decltype(kc)::value)) * d;
    });
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6] = s1;
        red[kThreads / 64 + (threadIdx.x >> 6)] = s2;
    }
    __syncthreads();
    ws_hist(j, ws)[256LL * chunk + threadIdx.x] = hist[threadIdx.x];
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int k = 0; k < kThreads / 64; ++k) t += red[threadIdx.x * (kThreads / 64) + k];
        ws_adler(j, ws)[2LL * chunk + threadIdx.x] = t;
    }
}

// ------------------------------------------------------------------------------------------------ 2: table and scan
__device__ __forceinline__ uint32_t rev_bits(uint32_t code, int len) { return len ? __brev(code) >> (32 - len) : 0; }

__global__ void __launch_bounds__(kThreads) png_table_kernel(PngJob j) {
    __shared__ uint32_t cnt[kDeflateSyms], scnt[kDeflateSyms];
    __shared__ uint16_t ssym[kDeflateSyms];
    __shared__ uint8_t slen[kDeflateSyms + 3], len[kDeflateSyms + 3];
    __shared__ DeflateScratch scratch;
    __shared__ uint32_t blc[16], next_code[16], wsum[kThreads / 64], hdr[kHeaderDwords];
    __shared__ unsigned long long ared[2 * (kThreads / 64)];
    __shared__ int m_sh;
    const int t = threadIdx.x;
    const long long b = blockIdx.x;
    uint32_t* ws = j.work + b * j.work_words;
    uint32_t* slot = j.out + b * j.slot_dwords;
    const uint32_t* hist = ws_hist(j, ws);

    {  // the image's histogram, and one end-of-block
        uint32_t tot = 0;
        for (uint32_t c = 0; c < j.nchunks; ++c) tot += hist[256LL * c + t];
        cnt[t] = tot;
        if (t == 0) cnt[256] = 1;
    }
    if (t < kHeaderDwords) hdr[t] = 0;
    __syncthreads();
    // rank sort of the non-zero counts: ascending, ties by symbol (esm_deflate_code_lengths' order)
    for (int i = t; i < kDeflateSyms; i += kThreads) {
        const uint32_t ci = cnt[i];
        int rank = 0, m = 0;
        for (int k = 0; k < kDeflateSyms; ++k) {
            const uint32_t ck = cnt[k];
            m += ck != 0;
            rank += ck != 0 && (ck < ci || (ck == ci && k < i));
        }
        if (ci) {
            scnt[rank] = ci;
            ssym[rank] = static_cast<uint16_t>(i);
        } else {
            len[i] = 0;
        }
        if (i == 0) m_sh = m;
    }
    __syncthreads();
    const int m = m_sh;  // >= 2: an image has at least its first filter byte, and end-of-block
    if (t == 0) deflate_lengths_sorted(scnt, m, slen, scratch);
    __syncthreads();
    for (int i = t; i < m; i += kThreads) len[ssym[i]] = slen[i];
    __syncthreads();
    // canonical codes (RFC 1951 3.2.2)
    if (t < 16) {
        uint32_t n = 0;
        if (t > 0)
            for (int k = 0; k < kDeflateSyms; ++k) n += len[k] == t;
        blc[t] = n;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t code = 0;
        next_code[0] = 0;
        for (int l = 1; l <= kDeflateMaxLen; ++l) {
            code = (code + blc[l - 1]) << 1;
            next_code[l] = code;
        }
    }
    __syncthreads();
    for (int i = t; i < kDeflateSyms; i += kThreads) {
        const int l = len[i];
        uint32_t code = next_code[l];
        for (int k = 0; k < i; ++k) code += len[k] == l;
        ws_table(j, ws)[i] = rev_bits(code, l) | static_cast<uint32_t>(l) << 16;
    }
    // the header image: 78 01, the 17 + 57 fixed bits, then 258 lengths as bit-reversed 4-bit codes from bit 90
    for (int i = t; i < 258; i += kThreads) {
        const uint32_t l = i < kDeflateSyms ? len[i] : 1;  // (the one distance code)
        const uint32_t v = __brev(l) >> 28;
        const int pos = 90 + 4 * i;
        atomicOr(&hdr[pos >> 5], v << (pos & 31));
        if ((pos & 31) > 28) atomicOr(&hdr[(pos >> 5) + 1], v >> (32 - (pos & 31)));
    }
    if (t == 0) {
        // BFINAL 1, BTYPE 2, HLIT 0, HDIST 0, HCLEN 15; then 19 x 3 bits in the order 16 17 18 0 8 7 ...: 0 0 0 4 ...
        unsigned long long fixed = 0x78ull | 0x01ull << 8 | (5ull | 15ull << 13) << 16;
        atomicOr(&hdr[0], static_cast<uint32_t>(fixed));
        unsigned long long cl = 0;
        for (int k = 3; k < 19; ++k) cl |= 4ull << (3 * k);
        // bits 33 .. 89
        atomicOr(&hdr[1], static_cast<uint32_t>(fixed >> 32) | static_cast<uint32_t>(cl << 1));
        atomicOr(&hdr[2], static_cast<uint32_t>(cl >> 31));
    }
    // each chunk's bit count, a wave per chunk: sum hist * len (the last chunk also carries end-of-block)
    uint32_t* offs = ws_offs(j, ws);
    {
        const int lane = t & 63, wave = t >> 6;
        uint32_t l4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) l4[k] = len[lane + 64 * k];
        for (uint32_t c = wave; c < j.nchunks; c += kThreads / 64) {
            uint32_t bits = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) bits += hist[256LL * c + lane + 64 * k] * l4[k];
            bits = wave_sum(bits);
            if (lane == 0) offs[c] = bits + (c == j.nchunks - 1 ? len[256] : 0);
        }
    }
    __syncthreads();  // (offs is read back by other lanes of this workgroup)
    // scan into bit offsets; zero the dword each chunk starts in (launch 3 ORs into it from both sides)
    uint32_t carry = kPreBits;
    for (uint32_t c0 = 0; c0 < j.nchunks; c0 += kThreads) {
        const uint32_t c = c0 + t;
        const uint32_t bits = c < j.nchunks ? offs[c] : 0;
        uint32_t total;
        const uint32_t off = carry + block_scan<kThreads>(bits, wsum, total);
        if (c < j.nchunks) {
            offs[c] = off;
            store_slot(j, slot, off >> 5, 0);
        }
        carry += total;
    }
    const uint32_t total_bits = carry;                  // < 2^32: raw < 2^28 and 15 bits a symbol
    const uint32_t trailer = (total_bits >> 3) + ((total_bits & 7) != 0);  // byte position of the Adler-32
    const uint32_t length = trailer + 4;
    for (long long d = (total_bits >> 5) + t; d <= (length - 1) >> 2; d += kThreads) store_slot(j, slot, d, 0);
    // Adler-32 (RFC 1950): s1 = 1 + sum d, s2 = N + sum (N - i) d, mod 65521; a chunk's share of s2 is its own
    // sum (n - i) d plus (N - end of the chunk) * its sum d.  64-bit, reduced term by term.
    unsigned long long s1 = 0, s2 = 0;
    const uint32_t* ad = ws_adler(j, ws);
    for (uint32_t c = t; c < j.nchunks; c += kThreads) {
        const unsigned long long a = ad[2LL * c], bb = ad[2LL * c + 1];
        const unsigned long long end = min(static_cast<unsigned long long>(c + 1) * kChunk,
                                           static_cast<unsigned long long>(j.raw));
        s1 += a;                                             // <= 2^28 * 255 over the whole image
        s2 = (s2 + bb + ((j.raw - end) % kAdlerMod) * (a % kAdlerMod)) % kAdlerMod;
    }
    for (int d = 32; d >= 1; d >>= 1) {
        s1 += __shfl_xor(s1, d);
        s2 += __shfl_xor(s2, d);
    }
    if ((t & 63) == 0) {
        ared[t >> 6] = s1;
        ared[kThreads / 64 + (t >> 6)] = s2;
    }
    __threadfence();
    __syncthreads();  // the zeroes are out before anything is stored or ORed over them
    if (t < kHeaderDwords) store_slot(j, slot, t, hdr[t]);
    __threadfence();
    __syncthreads();
    if (t == 0) {
        s1 = 1;
        s2 = j.raw;
        for (int k = 0; k < kThreads / 64; ++k) {
            s1 += ared[k];
            s2 += ared[kThreads / 64 + k];
        }
        const uint32_t adler = static_cast<uint32_t>(s2 % kAdlerMod) << 16 | static_cast<uint32_t>(s1 % kAdlerMod);
        // big-endian, at any byte position: OR into the dwords zeroed above
        for (int k = 0; k < 4; ++k) {
            const uint32_t pos = trailer + k;
            or_slot(j, slot, pos >> 2, ((adler >> (24 - 8 * k)) & 0xFF) << (8 * (pos & 3)));
        }
        uint32_t* meta = ws_table(j, ws) + kTableWords;
        meta[0] = total_bits;
        meta[1] = trailer;
        j.lengths[b] = static_cast<int32_t>(length);
    }
}

// ---------------------------------------------------------------------------------------------------------- 3: emit
__device__ __forceinline__ void stage_or(uint32_t* stage, uint32_t pos, unsigned long long v) {
    const uint32_t i = pos >> 5, sh = pos & 31;
    if (i + 2 >= static_cast<uint32_t>(kStageDwords)) return;  // (never taken with a sound offset)
    const unsigned long long lo = v << sh;
    const uint32_t hi = sh ? static_cast<uint32_t>(v >> (64 - sh)) : 0;
    if (static_cast<uint32_t>(lo)) atomicOr(&stage[i], static_cast<uint32_t>(lo));
    if (static_cast<uint32_t>(lo >> 32)) atomicOr(&stage[i + 1], static_cast<uint32_t>(lo >> 32));
    if (hi) atomicOr(&stage[i + 2], hi);
}

template <int KIND>
__global__ void __launch_bounds__(kThreads) png_emit_kernel(PngJob j) {
    __shared__ uint32_t stage[kStageDwords];
    __shared__ uint32_t table[kDeflateSyms];
    __shared__ uint32_t wsum[kThreads / 64];
    const uint32_t chunk = blockIdx.x;
    const long long b = blockIdx.y;
    const int t = threadIdx.x;
    uint32_t* ws = j.work + b * j.work_words;
    uint32_t* slot = j.out + b * j.slot_dwords;
    for (int i = t; i < kStageDwords; i += kThreads) stage[i] = 0;
    for (int i = t; i < kDeflateSyms; i += kThreads) table[i] = ws_table(j, ws)[i];
    const uint32_t start = ws_offs(j, ws)[chunk];
    __syncthreads();
    unsigned long long word[4] = {0, 0, 0, 0};
    uint32_t nb[4] = {0, 0, 0, 0};
    for_filtered<KIND>(j, b, chunk, [&](auto kc, uint32_t d) {
        constexpr int g = decltype(kc)::value / 4;
        const uint32_t e = table[d];
        word[g] |= static_cast<unsigned long long>(e & 0xFFFF) << nb[g];
        nb[g] += e >> 16;
    });
    uint32_t total;
    uint32_t pos = (start & 31) + block_scan<kThreads>(nb[0] + nb[1] + nb[2] + nb[3], wsum, total);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        if (nb[g]) stage_or(stage, pos, word[g]);
        pos += nb[g];
    }
    if (chunk == j.nchunks - 1) {  // end-of-block behind the last symbol
        const uint32_t e = table[256];
        if (t == 0) stage_or(stage, (start & 31) + total, e & 0xFFFF);
        total += e >> 16;
    }
    __syncthreads();
    const uint32_t end = (start & 31) + total;  // in bits from the first dword of the chunk
    const uint32_t nd = (end + 31) >> 5;
    const long long d0 = start >> 5;
    for (uint32_t i = t; i < nd && i < static_cast<uint32_t>(kStageDwords); i += kThreads) {
        const bool interior = (i > 0 || (start & 31) == 0) && 32 * (i + 1) <= end;
        if (interior)
            store_slot(j, slot, d0 + i, stage[i]);
        else
            or_slot(j, slot, d0 + i, stage[i]);
    }
}

int validate(const char* what, int B, int rows, int w, int bpp, const void* src, const void* work, const void* out,
             long long slot_stride, const void* lengths, int filter, PngJob& j) {
    const std::string p = std::string(what) + ": ";
    if (filter < 0 || filter > 2) return arg_error(p + "unknown filter (0 None, 1 Sub, 2 Up)");
    if (B <= 0 || rows <= 0 || w <= 0) return arg_error(p + "non-positive size");
    if (B > 65535) return arg_error(p + "B > 65535");
    const long long raw = static_cast<long long>(rows) * (1LL + static_cast<long long>(bpp) * w);
    if (raw >= kMaxRaw) return arg_error(p + "raw bytes per image >= 2^28 (bit offsets are 32-bit)");
    if (slot_stride < esm_png_stream_bound(raw)) return arg_error(p + "slot smaller than esm_png_stream_bound");
    if (slot_stride % 4) return arg_error(p + "slot stride is not a multiple of 4");
    if (!src || !work || !out || !lengths) return arg_error(p + "null pointer");
    if (reinterpret_cast<uintptr_t>(out) % 4 || reinterpret_cast<uintptr_t>(work) % 4)
        return arg_error(p + "out / work not 4-byte aligned");
    j = PngJob{};
    j.src = src;
    j.work = static_cast<uint32_t*>(const_cast<void*>(work));
    j.out = static_cast<uint32_t*>(const_cast<void*>(out));
    j.lengths = static_cast<int32_t*>(const_cast<void*>(lengths));
    j.rows = rows;
    j.w = w;
    j.row_raw = 1 + bpp * w;
    j.raw = static_cast<uint32_t>(raw);
    j.nchunks = static_cast<uint32_t>((raw + kChunk - 1) / kChunk);
    j.work_words = work_words(j.nchunks);
    j.slot_dwords = slot_stride / 4;
    j.filter = filter;
    return ESM_OK;
}

template <int KIND>
int launch(const PngJob& j, int B, const char* what, hipStream_t s) {
    const dim3 grid(j.nchunks, B);
    hipLaunchKernelGGL(png_count_kernel<KIND>, grid, dim3(kThreads), 0, s, j);
    hipLaunchKernelGGL(png_table_kernel, dim3(B), dim3(kThreads), 0, s, j);
    hipLaunchKernelGGL(png_emit_kernel<KIND>, grid, dim3(kThreads), 0, s, j);
    return check_launch(what);
}

}  // namespace
}  // namespace esm

extern "C" {

int esm_png_chunk_bytes(void) { return esm::kChunk; }

long long esm_png_stream_bound(long long raw_bytes) {
    if (raw_bytes <= 0 || raw_bytes >= esm::kMaxRaw) return ESM_ERR_ARG;
    const long long bits = esm::kHeaderBits + 9 * (raw_bytes + 1);
    return (2 + (bits + 7) / 8 + 4 + 15) / 16 * 16;
}

long long esm_png_workspace_bytes(int B, int rows, int row_bytes) {
    if (B <= 0 || rows <= 0 || row_bytes <= 0) return ESM_ERR_ARG;
    const long long raw = static_cast<long long>(rows) * (1LL + row_bytes);
    if (raw >= esm::kMaxRaw) return ESM_ERR_ARG;
    return 4 * B * esm::work_words((raw + esm::kChunk - 1) / esm::kChunk);
}

int esm_deflate_code_lengths(const uint32_t hist[257], uint8_t len[257]) {
    if (!hist || !len) return esm::arg_error("deflate_code_lengths: null pointer");
    uint32_t cnt[esm::kDeflateSyms];
    uint16_t sym[esm::kDeflateSyms];
    uint8_t sorted[esm::kDeflateSyms];
    unsigned long long sum = 0;
    int m = 0;
    for (int i = 0; i < esm::kDeflateSyms; ++i) {
        const uint32_t c = i == 256 && hist[i] == 0 ? 1 : hist[i];  // end-of-block always gets a code
        sum += c;
        len[i] = 0;
        if (c) sym[m++] = static_cast<uint16_t>(i);
    }
    if (sum >> 32) return esm::arg_error("deflate_code_lengths: the counts sum to 2^32 or more");
    auto count = [&](int i) { return i == 256 && hist[i] == 0 ? 1u : hist[i]; };
    std::stable_sort(sym, sym + m, [&](uint16_t a, uint16_t b) { return count(a) < count(b); });
    if (m == 1) {  // nothing but end-of-block: a second, unused code keeps the code complete
        len[256] = len[0] = 1;
        return ESM_OK;
    }
    for (int i = 0; i < m; ++i) cnt[i] = count(sym[i]);
    esm::DeflateScratch scratch;
    esm::deflate_lengths_sorted(cnt, m, sorted, scratch);
    for (int i = 0; i < m; ++i) len[sym[i]] = sorted[i];
    return ESM_OK;
}

int esm_deflate_header(const uint8_t len[257], uint8_t out[139], int* nbits) {
    if (!len || !out) return esm::arg_error("deflate_header: null pointer");
    for (int i = 0; i < esm::kDeflateSyms; ++i)
        if (len[i] > esm::kDeflateMaxLen) return esm::arg_error("deflate_header: a length above 15");
    for (int i = 0; i < 139; ++i) out[i] = 0;
    int pos = 0;
    auto put = [&](uint32_t v, int n) {  // n bits of v, least significant first
        for (int k = 0; k < n; ++k, ++pos) out[pos >> 3] |= static_cast<uint8_t>(((v >> k) & 1) << (pos & 7));
    };
    auto put_code = [&](uint32_t code, int n) {  // a Huffman code: most significant bit first
        for (int k = n - 1; k >= 0; --k, ++pos) out[pos >> 3] |= static_cast<uint8_t>(((code >> k) & 1) << (pos & 7));
    };
    put(1, 1);   // BFINAL
    put(2, 2);   // BTYPE: dynamic Huffman
    put(0, 5);   // HLIT: 257 codes
    put(0, 5);   // HDIST: 1 code
    put(15, 4);  // HCLEN: 19 lengths
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int k = 0; k < 19; ++k) put(order[k] < 16 ? 4 : 0, 3);
    for (int i = 0; i < esm::kDeflateSyms; ++i) put_code(len[i], 4);  // symbol s of the length code is the code s
    put_code(1, 4);                                                    // the one distance code: length 1
    if (nbits) *nbits = pos;
    return ESM_OK;
}

int esm_png_encode_u16(const uint16_t* src, int B, int h, int w, void* work, uint8_t* out, long long slot_stride,
                       int32_t* lengths, int filter, void* stream) {
    esm::PngJob j;
    if (int rc = esm::validate("png_encode_u16", B, h, w, 2, src, work, out, slot_stride, lengths, filter, j)) return rc;
    j.src_image = static_cast<long long>(h) * w;
    return esm::launch<esm::SRC_U16>(j, B, "png_encode_u16", esm::as_stream(stream));
}

int esm_png_encode_rgb8(const uint8_t* src, int B, int h, int w, int bgr, void* work, uint8_t* out,
                        long long slot_stride, int32_t* lengths, int filter, void* stream) {
    esm::PngJob j;
    if (int rc = esm::validate("png_encode_rgb8", B, h, w, 3, src, work, out, slot_stride, lengths, filter, j)) return rc;
    j.src_image = 3LL * h * w;
    j.bgr = bgr != 0;
    return esm::launch<esm::SRC_RGB8>(j, B, "png_encode_rgb8", esm::as_stream(stream));
}

int esm_png_encode_disp_f32(const float* disp, int B, int Hp, int Wp, int top, int left, int h, int w, void* work,
                            uint8_t* out, long long slot_stride, int32_t* lengths, int filter, void* stream) {
    esm::PngJob j;
    if (int rc = esm::validate("png_encode_disp_f32", B, h, w, 2, disp, work, out, slot_stride, lengths, filter, j))
        return rc;
    if (Hp <= 0 || Wp <= 0) return esm::arg_error("png_encode_disp_f32: non-positive size");
    if (top < 0 || left < 0 || top + static_cast<long long>(h) > Hp || left + static_cast<long long>(w) > Wp)
        return esm::arg_error("png_encode_disp_f32: window outside the map");
    j.src_image = static_cast<long long>(Hp) * Wp;
    j.pitch = Wp;
    j.top = top;
    j.left = left;
    return esm::launch<esm::SRC_DISP>(j, B, "png_encode_disp_f32", esm::as_stream(stream));
}

}  // extern "C"
