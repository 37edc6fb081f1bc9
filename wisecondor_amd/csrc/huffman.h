// Length-limited Huffman code lengths for the deflate encoder (deflate.hip): one serial routine for host and device.
// The device calls it from one thread with the workspace in LDS (a private array would live in scratch memory); the
// host entry wc_huffman_lengths calls the same code, which is how it is tested without a GPU.
#pragma once
#include <stdint.h>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace wc {

const int HUFF_MAX_SYMS = 288;      // deflate's largest alphabet (286 literal/length symbols), padded

struct HuffWork {
    uint64_t weight[HUFF_MAX_SYMS];         // internal nodes in the order they are made: their weights never decrease
    uint32_t cnt[256];                      // radix sort: digit counts
    uint32_t bl[16];                        // leaves per code length
    uint16_t order[2][HUFF_MAX_SYMS];       // used symbols, sorted by frequency (two buffers of the radix sort)
    uint16_t parent[2 * HUFF_MAX_SYMS];     // [k < m] of sorted leaf k, [m + i] of internal node i: an internal node's number
    uint16_t depth[HUFF_MAX_SYMS];          // of the internal nodes
};

// len[s] = code length of symbol s (0: freq[s] == 0) of an optimal prefix code whose lengths are limited to `limit` bits.
//   - the used symbols are sorted by (frequency, symbol) and merged with the two-queue construction;
//   - leaves deeper than `limit` are clamped to it, which over-subscribes the code by a whole number E of 2^-limit;
//     E times, a leaf of the longest length below the limit gets one of the clamped leaves as its sibling one level down
//     (-2^-b + 2 * 2^-(b+1) - 2^-limit: exactly one unit each, zlib's gen_bitlen move), so the Kraft sum ends at 1;
//   - the lengths are handed out again along the sorted order, longest to rarest: never dearer than the tree's own
//     assignment, so where nothing was clamped the cost is the unlimited Huffman cost.
// One used symbol gets length 1.  n <= HUFF_MAX_SYMS, 1 <= limit <= 15, and the used symbols must number at most 2^limit.
__host__ __device__ inline void huffman_lengths(const uint32_t *freq, int n, int limit, uint8_t *len, HuffWork &w) {
    int m = 0;
    uint32_t maxf = 0;
    for (int s = 0; s < n; ++s) {
        len[s] = 0;
        if (freq[s]) {
            w.order[0][m++] = (uint16_t)s;
            if (freq[s] > maxf) maxf = freq[s];
        }
    }
    if (m == 0) return;
    if (m == 1) { len[w.order[0][0]] = 1; return; }
    int cur = 0;
    for (int shift = 0; shift < 32 && (maxf >> shift); shift += 8) {        // stable: ties stay in symbol order
        for (int i = 0; i < 256; ++i) w.cnt[i] = 0;
        for (int i = 0; i < m; ++i) w.cnt[(freq[w.order[cur][i]] >> shift) & 255u]++;
        uint32_t at = 0;
        for (int i = 0; i < 256; ++i) { const uint32_t c = w.cnt[i]; w.cnt[i] = at; at += c; }
        for (int i = 0; i < m; ++i) {
            const uint16_t s = w.order[cur][i];
            w.order[cur ^ 1][w.cnt[(freq[s] >> shift) & 255u]++] = s;
        }
        cur ^= 1;
    }
    const uint16_t *ord = w.order[cur];
    int leaf = 0, inode = 0;                    // heads of the two queues: sorted leaves, internal nodes inode .. made - 1
    for (int made = 0; made < m - 1; ++made) {
        uint64_t sum = 0;
        for (int k = 0; k < 2; ++k) {
            if (leaf < m && (inode >= made || (uint64_t)freq[ord[leaf]] <= w.weight[inode])) {
                sum += freq[ord[leaf]];
                w.parent[leaf++] = (uint16_t)made;
            } else {
                sum += w.weight[inode];
                w.parent[m + inode++] = (uint16_t)made;
            }
        }
        w.weight[made] = sum;
    }
    w.depth[m - 2] = 0;                         // the root; a node's parent is made after it
    for (int i = m - 3; i >= 0; --i) w.depth[i] = (uint16_t)(w.depth[w.parent[m + i]] + 1);
    for (int b = 0; b < 16; ++b) w.bl[b] = 0;
    uint64_t kraft = 0;                         // in units of 2^-limit
    for (int k = 0; k < m; ++k) {
        int d = w.depth[w.parent[k]] + 1;
        if (d > limit) d = limit;
        w.bl[d]++;
        kraft += 1ull << (limit - d);
    }
    for (uint64_t over = kraft - (1ull << limit); over > 0; --over) {
        int bits = limit - 1;
        while (bits > 0 && w.bl[bits] == 0) --bits;
        if (bits == 0) break;                   // (more used symbols than 2^limit codes: the caller's error)
        w.bl[bits]--;
        w.bl[bits + 1] += 2;
        w.bl[limit]--;
    }
    int pos = 0;
    for (int bits = limit; bits >= 1; --bits)
        for (uint32_t c = w.bl[bits]; c > 0 && pos < m; --c) len[ord[pos++]] = (uint8_t)bits;
}

}  // namespace wc
