// Huffman code lengths for a literal-only deflate block (RFC 1951 section 3.2.2): at most 15 bits, and always a
// COMPLETE code (the Kraft sum is exactly 1; zlib's inflate rejects an incomplete or over-subscribed literal code).
// One function for both sides: esm_deflate_code_lengths (the host export, csrc/png.hip) and lane 0 of the
// per-image table kernel run it on the same sorted counts, so the device's table is the host's, bit for bit.
#pragma once

#include <cstdint>

namespace esm {

constexpr int kDeflateSyms = 257;   // literals 0-255 and end-of-block
constexpr int kDeflateMaxLen = 15;

struct DeflateScratch {
    uint32_t w[kDeflateSyms - 1];           // weights of the internal nodes, in creation order
    uint16_t parent[2 * kDeflateSyms - 1];  // leaves 0 .. m-1, then internal nodes m .. 2m-2
    uint16_t depth[kDeflateSyms - 1];
    uint16_t num[kDeflateMaxLen + 1];
};

// cnt[0 .. m): the non-zero counts in ascending order (ties in any fixed order), 2 <= m <= 257, their sum < 2^32.
// len[i] receives the code length of cnt[i].
//   1. The two-queue Huffman merge: leaves are consumed in order, internal nodes are created in non-decreasing
//      weight, so both queues stay sorted and every step is two compares: m - 1 steps.  On a tie the LEAF is
//      taken first, which gives the shallowest of the optimal trees: if any optimal tree fits 15 bits, this one does.
//   2. A tree deeper than 15 (Fibonacci-like counts; a Sub-filtered disparity of a few hundred KB does reach it):
//      the lengths' histogram is folded at 15 and the Kraft excess is removed one unit at a time (a 15-bit code is
//      dropped and re-attached beside the deepest code shorter than 15, which moves down one level), then the
//      lengths are handed out again by rank, longest to rarest.
//   3. The result of 2 is not optimal, so it is compared with the flat complete code over the m symbols
//      (floor(log2 m) bits, the 2 (m - 2^k) rarest one bit more) and the cheaper one is kept: the body never costs
//      more than 8 bits a symbol plus one more for the two rarest, which is what esm_png_stream_bound assumes.
__host__ __device__ inline void deflate_lengths_sorted(const uint32_t* cnt, int m, uint8_t* len, DeflateScratch& s) {
    int li = 0, ni = 0;
    for (int nn = 0; nn < m - 1; ++nn) {
        uint32_t sum = 0;
        for (int t = 0; t < 2; ++t) {
            const bool leaf = li < m && (ni >= nn || cnt[li] <= s.w[ni]);
            if (leaf) {
                sum += cnt[li];
                s.parent[li++] = static_cast<uint16_t>(m + nn);
            } else {
                sum += s.w[ni];
                s.parent[m + ni++] = static_cast<uint16_t>(m + nn);
            }
        }
        s.w[nn] = sum;
    }
    s.depth[m - 2] = 0;  // the root
    for (int nn = m - 3; nn >= 0; --nn) s.depth[nn] = static_cast<uint16_t>(s.depth[s.parent[m + nn] - m] + 1);
    int deepest = 0;
    for (int i = 0; i < m; ++i) {
        const int d = s.depth[s.parent[i] - m] + 1;
        deepest = d > deepest ? d : deepest;
        len[i] = static_cast<uint8_t>(d > kDeflateMaxLen ? kDeflateMaxLen : d);
    }
    if (deepest <= kDeflateMaxLen) return;

    for (int l = 0; l <= kDeflateMaxLen; ++l) s.num[l] = 0;
    for (int i = 0; i < m; ++i) ++s.num[len[i]];
    uint32_t total = 0;
    for (int l = 1; l <= kDeflateMaxLen; ++l) total += static_cast<uint32_t>(s.num[l]) << (kDeflateMaxLen - l);
    while (total > (1u << kDeflateMaxLen)) {
        --s.num[kDeflateMaxLen];
        for (int l = kDeflateMaxLen - 1; l >= 1; --l)
            if (s.num[l]) {
                --s.num[l];
                s.num[l + 1] = static_cast<uint16_t>(s.num[l + 1] + 2);
                break;
            }
        --total;
    }
    uint64_t cost = 0;
    for (int i = 0, l = kDeflateMaxLen; i < m; ++i) {
        while (s.num[l] == 0) --l;
        --s.num[l];
        len[i] = static_cast<uint8_t>(l);
        cost += static_cast<uint64_t>(cnt[i]) * l;
    }
    int k = 0;
    while ((2 << k) <= m) ++k;  // floor(log2 m)
    const int longer = 2 * (m - (1 << k));
    uint64_t flat = 0;
    for (int i = 0; i < m; ++i) flat += static_cast<uint64_t>(cnt[i]) * (i < longer ? k + 1 : k);
    if (flat < cost)
        for (int i = 0; i < m; ++i) len[i] = static_cast<uint8_t>(i < longer ? k + 1 : k);
}

}  // namespace esm
