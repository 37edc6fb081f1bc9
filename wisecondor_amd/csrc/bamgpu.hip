// Device stage of the BAM reader: the compressed bytes of a whole file (host stage: bamfile.cpp) go to the device, where
//   k_bg_inflate   one BGZF block per wave: raw deflate (stored / fixed / dynamic Huffman) into the block's place in one
//                  contiguous inflated buffer, then the block's CRC-32 (sliced over the lanes, slices combined by
//                  multiplication with x^(8 n) modulo the CRC polynomial); one status word per block
//   k_bg_chain     record starts, by the block_size chain alone: per segment of BG_SEG inflated bytes, from its end towards
//                  its start (a record is at least 36 bytes, so 36 consecutive offsets depend only on higher ones: 36
//                  offsets per wave step), the map  entry offset -> where that chain leaves the segment
//   k_bg_link      one wave walks the segments from the first record: the entry offset of every segment on the real chain
//   k_bg_walk      one lane per segment follows the real chain through its segment: the record rule of bamfile.h and the
//                  counters of bamio.cpp's Parser::feed; <false> counts the placed records, <true> (after k_bg_scan)
//                  writes their fields in file order
//   k_bg_order / k_bg_offsets   the coordinate-order check on neighbouring placed records, the per-reference offsets
// The streamed reader (wc_bam_stream_dev, at the end) sends the file through the same kernels chunk by chunk: the walk
// takes a `last` flag (data that is not the file's end may end inside a record: the carry), and the order check, the
// per-reference counts and the running base of the output live in device words (BG_*) that k_bg_begin / k_bg_advance
// keep across chunks.  To these kernels the whole file is one chunk, the last, with nothing before it.
// Every loop is bounded by the bytes that are there (see the comments at the loops); a violation sets a status and the
// wave stops.  The inflate kernel's back-references read the global output it has written itself: its LDS holds the
// Huffman tables only ("convert: the device reader").
#include <limits.h>

#include <algorithm>
#include <chrono>

#include "bamfile.h"
#include "ctx.h"

namespace {

const int BG_SEG = 65536;           // inflated bytes per segment of the record chain; offsets inside fit 16 bits
const int BG_STEP = 36;             // the least record: block_size >= 32 plus its own 4 bytes
const unsigned BG_FAR = 0xFFFEu;    // map word: the chain leaves the segment by 65 534 bytes or more (a record that long)
const unsigned BG_BAD = 0xFFFFu;    // map word: the chain reaches a block_size below 32 or cut off by the end of the data
const int BG_LIT_BITS = 10, BG_DIST_BITS = 9, BG_CL_BITS = 7;
const double BG_BUDGET_FRACTION = 0.8;      // of the free device memory, when the caller names no budget

enum { BG_E_DEFLATE = 1, BG_E_CRC = 2 };

// The walk's device words, kept across the chunks of a streamed open:
// [0..2] mapped, unmapped, no_coordinate (all chunks)   [3] placed records of this chunk (k_bg_scan)
// [4] record error, (file-absolute inflated offset << 3 | wc::BAM_R_* kind)
// [5] order error, (placed index in the file << 2 | kind)   [6] placed records of the chunks before
// [7] offset in carry + chunk of the first record that does not end inside   [8] reference of the last placed record so far
enum { BG_PLACED = 3, BG_RECERR = 4, BG_ORDERR = 5, BG_BASE = 6, BG_TAIL = 7, BG_LASTREF = 8, BG_WORDS = 16 };

struct InflLds {
    uint32_t crc_tab[256];
    uint32_t lit_count[16], dist_count[16];
    uint16_t lit[1 << BG_LIT_BITS];
    uint16_t dist[1 << BG_DIST_BITS];           // the code-length code's table while a dynamic header is read
    uint16_t lit_sorted[288];
    uint16_t dist_sorted[32];
    uint8_t lens[320];
    uint8_t cl_lens[20];
};

__constant__ uint8_t bg_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// a * b modulo the CRC-32 polynomial, reflected bit order (bit 31 is x^0): zlib's multmodp
__device__ __forceinline__ uint32_t bg_multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
#pragma unroll 1
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
    }
    return p;
}

// Canonical Huffman tables of `n` code lengths (LDS): `table` has 2^tbits entries (symbol << 4 | length; 0: the code is
// longer than tbits, or absent), count[len] / sorted[] serve the longer codes as in zlib's puff.  Lane L assigns the codes
// of length L.  Returns nonzero (in every lane) for an over-subscribed set, and for an incomplete one as zlib's
// inflate_table judges it.  All 64 lanes call this together.
__device__ __noinline__ int bg_build(const uint8_t *lens, int n, uint16_t *table, int tbits, uint32_t *count, uint16_t *sorted, bool strict,
                        int lane) {
    for (int i = lane; i < (1 << tbits); i += 64) table[i] = 0;
    if (lane < 16) count[lane] = 0;
    wc_sync();
    for (int s = lane; s < n; s += 64) {
        const int l = lens[s];
        if (l) atomicAdd(&count[l], 1u);
    }
    wc_sync();
    int left = 1, maxlen = 0;
    bool over = false;
#pragma unroll 1
    for (int l = 1; l <= 15; ++l) {
        const int c = (int)count[l];
        left = (left << 1) - c;
        if (left < 0) { over = true; left = 0; }
        if (c) maxlen = l;
    }
    if (over || (left > 0 && maxlen != 0 && (strict || maxlen != 1))) return 1;
    if (lane >= 1 && lane <= 15 && count[lane]) {
        uint32_t code = 0, offs = 0;
        for (int b = 1; b <= lane; ++b) {
            code = (code + (b > 1 ? count[b - 1] : 0u)) << 1;
            if (b < lane) offs += count[b];
        }
        for (int s = 0; s < n; ++s) {
            if (lens[s] != lane) continue;
            sorted[offs++] = (uint16_t)s;           // offs < n: the counts sum to at most n
            if (lane <= tbits) {
                const uint32_t rev = __brev(code) >> (32 - lane);
                for (uint32_t e = rev; e < (1u << tbits); e += 1u << lane) table[e] = (uint16_t)((s << 4) | lane);
            }
            ++code;
        }
    }
    wc_sync();
    return 0;
}

// One symbol: at least one bit is consumed, or -1 is returned.  The caller has 15 bits or more in the buffer.
__device__ __forceinline__ int bg_decode(uint64_t &bb, int &bc, const uint16_t *table, int tbits, const uint32_t *count,
                                         const uint16_t *sorted) {
    const uint32_t e = (uint32_t)__builtin_amdgcn_readfirstlane((int)table[(uint32_t)bb & ((1u << tbits) - 1u)]);
    const int l = (int)(e & 15u);
    if (l) {
        bb >>= l;
        bc -= l;
        return (int)(e >> 4);
    }
    int code = 0, first = 0, index = 0;
#pragma unroll 1
    for (int len = 1; len <= 15; ++len) {
        code |= (int)((bb >> (len - 1)) & 1u);
        const int c = (int)count[len];
        if (code - c < first) {
            bb >>= len;
            bc -= len;
            return (int)sorted[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

__global__ void __launch_bounds__(64) k_bg_inflate(const uint8_t *__restrict__ comp, const wc::BgzfBlock *__restrict__ dir,
                                                   uint8_t *plain, int *__restrict__ status) {
    __shared__ InflLds S;
    const int lane = threadIdx.x;
    const wc::BgzfBlock blk = dir[blockIdx.x];
    const uint8_t *in = comp + blk.in_off;
    uint8_t *dst = plain + blk.out_off;
    const int in_len = blk.in_len, isize = (int)blk.isize;
    const int in_bits = 8 * in_len;                 // in_len < 65536: BSIZE has 16 bits
    const int skip0 = (int)((uintptr_t)in & 3);
    const uint32_t *inw = reinterpret_cast<const uint32_t *>(in - skip0);   // aligned words; comp itself is aligned
    const int lim_bytes = skip0 + in_len + 8;       // no load starts here or beyond (WC_BGZF_PAD covers the last block)

    for (int k = 0; k < 4; ++k) {
        uint32_t c = (uint32_t)(lane * 4 + k);
        for (int j = 0; j < 8; ++j) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
        S.crc_tab[lane * 4 + k] = c;
    }

    // the bit reader: aligned 32-bit words; `loaded` counts the block's own bits that have entered the buffer, so
    // loaded - bc bits are consumed.  Words from lim_bytes on are zeros: whoever consumes them fails the check below.
    uint64_t bb = 0;
    int bc = 0, loaded = 0, wi = 0;
    auto init = [&](int bytepos) {                  // 0 <= bytepos <= in_len
        const int at = skip0 + bytepos, skip = (at & 3) * 8;
        wi = at >> 2;
        bb = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)inw[wi]) >> skip;
        ++wi;
        bc = 32 - skip;
        loaded = 8 * bytepos + bc;
    };
    auto refill = [&]() {                           // afterwards bc >= 33
        if (bc <= 32) {
            uint32_t w = 0;
            if (4 * wi < lim_bytes) w = (uint32_t)__builtin_amdgcn_readfirstlane((int)inw[wi]);
            ++wi;
            bb |= (uint64_t)w << bc;
            bc += 32;
            loaded += 32;
        }
    };
    auto bits = [&](int n) {
        const uint32_t v = (uint32_t)bb & ((1u << n) - 1u);
        bb >>= n;
        bc -= n;
        return (int)v;
    };

    int op = 0, err = 0;
    bool last = false;
    init(0);
    // every pass consumes the 3 header bits; the test at the head ends the loop once the block's bits are used up
    while (!last && !err) {
        if (loaded - bc > in_bits) { err = 1; break; }
        refill();
        last = bits(1) != 0;
        const int type = bits(2);
        if (type == 0) {
            bits(bc & 7);                           // to the byte boundary (loaded is a multiple of 8)
            refill();
            const int len = bits(16), nlen = bits(16);
            const int bytepos = (loaded - bc) >> 3;
            if ((len ^ 0xFFFF) != nlen || bytepos + len > in_len || op + len > isize) { err = 1; break; }
            for (int i = lane; i < len; i += 64) dst[op + i] = in[bytepos + i];
            op += len;
            init(bytepos + len);
            continue;
        }
        if (type == 3) { err = 1; break; }
        int n_lit = 288, n_dist = 30;
        if (type == 1) {
            for (int s = lane; s < 288; s += 64) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
            if (lane < 32) S.lens[288 + lane] = 5;     // 32 codes of 5 bits: a complete set; 30 and 31 are refused below
            n_dist = 32;
        } else {
            refill();
            n_lit = bits(5) + 257;
            n_dist = bits(5) + 1;
            const int n_cl = bits(4) + 4;
            if (n_lit > 286 || n_dist > 30) { err = 1; break; }
            if (lane < 19) S.cl_lens[lane] = 0;
            wc_sync();
            for (int i = 0; i < n_cl; ++i) {
                refill();
                const int v = bits(3);
                if (lane == 0) S.cl_lens[bg_cl_order[i]] = (uint8_t)v;
            }
            wc_sync();
            if (bg_build(S.cl_lens, 19, S.dist, BG_CL_BITS, S.dist_count, S.dist_sorted, true, lane)) { err = 1; break; }
            int i = 0, prev = 0;
            const int n_all = n_lit + n_dist;
            while (i < n_all) {                     // i grows in every pass
                if (loaded - bc > in_bits) { err = 1; break; }
                refill();
                const int s = bg_decode(bb, bc, S.dist, BG_CL_BITS, S.dist_count, S.dist_sorted);
                if (s < 0 || s > 18) { err = 1; break; }
                if (s < 16) {
                    if (lane == 0) S.lens[i] = (uint8_t)s;
                    prev = s;
                    ++i;
                    continue;
                }
                int rep, val = 0;
                if (s == 16) {
                    if (i == 0) { err = 1; break; }
                    val = prev;
                    rep = 3 + bits(2);
                } else if (s == 17) {
                    rep = 3 + bits(3);
                } else {
                    rep = 11 + bits(7);
                }
                if (i + rep > n_all) { err = 1; break; }
                for (int j = lane; j < rep; j += 64) S.lens[i + j] = (uint8_t)val;
                prev = val;
                i += rep;
            }
            if (err) break;
        }
        wc_sync();
        if (type == 2 && S.lens[256] == 0) { err = 1; break; }
        if (bg_build(S.lens, n_lit, S.lit, BG_LIT_BITS, S.lit_count, S.lit_sorted, false, lane)) { err = 1; break; }
        if (bg_build(S.lens + n_lit, n_dist, S.dist, BG_DIST_BITS, S.dist_count, S.dist_sorted, false, lane)) { err = 1; break; }
        // the symbols: every pass consumes a bit or more (bg_decode) or ends the loop
        for (;;) {
            if (loaded - bc > in_bits) { err = 1; break; }
            refill();
            const int sym = bg_decode(bb, bc, S.lit, BG_LIT_BITS, S.lit_count, S.lit_sorted);
            if (sym < 0) { err = 1; break; }
            if (sym < 256) {
                if (op >= isize) { err = 1; break; }
                if (lane == 0) dst[op] = (uint8_t)sym;
                ++op;
                continue;
            }
            if (sym == 256) break;
            if (sym > 285) { err = 1; break; }
            int len;
            if (sym < 265) {
                len = sym - 254;
            } else if (sym == 285) {
                len = 258;
            } else {
                const int eb = (sym - 261) >> 2;
                len = 3 + ((4 + ((sym - 265) & 3)) << eb) + bits(eb);
            }
            refill();
            const int ds = bg_decode(bb, bc, S.dist, BG_DIST_BITS, S.dist_count, S.dist_sorted);
            if (ds < 0 || ds > 29) { err = 1; break; }
            int dist;
            if (ds < 4) {
                dist = ds + 1;
            } else {
                const int eb = (ds >> 1) - 1;       // up to 13 bits; 15 + 13 <= the 33 bits refill() left
                dist = 1 + ((2 + (ds & 1)) << eb) + bits(eb);
            }
            if (dist > op || op + len > isize) { err = 1; break; }
            wc_sync();                              // this wave's earlier stores, before other lanes load them
            uint8_t *to = dst + op;
            const uint8_t *from = to - dist;        // every source byte lies below op: the lanes do not depend on each other
            for (int i = lane; i < len; i += 64) to[i] = from[dist >= len ? i : i % dist];
            op += len;
        }
    }
    if (!err && (op != isize || loaded - bc > in_bits)) err = 1;
    wc_sync();
    int st = err ? BG_E_DEFLATE : 0;
    if (!err) {
        const int slice = (isize + 63) / 64;
        const int begin = min(lane * slice, isize), end = min(begin + slice, isize);
        uint32_t c = 0;
        if (end > begin) {
            c = 0xFFFFFFFFu;
#pragma unroll 1
            for (int i = begin; i < end; ++i) c = S.crc_tab[(c ^ dst[i]) & 0xFFu] ^ (c >> 8);
            c ^= 0xFFFFFFFFu;
            // crc(A B) = crc(A) x^(8 |B|) + crc(B): this slice's share of the block's CRC
            uint32_t xp = 0x80000000u, b = 0x00800000u;         // x^0, x^8
            for (int n = isize - end; n; n >>= 1) {
                if (n & 1) xp = bg_multmodp(b, xp);
                b = bg_multmodp(b, b);
            }
            c = bg_multmodp(xp, c);
        }
        for (int m = 1; m < 64; m <<= 1) c ^= (uint32_t)__shfl_xor((int)c, m);
        if (c != blk.crc) st = BG_E_CRC;
    }
    if (lane == 0) status[blockIdx.x] = st;
}

__device__ __forceinline__ uint32_t bg_ld32(const uint8_t *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// map[a], a an absolute inflated offset of segment s = a / BG_SEG ending at e = min((s + 1) BG_SEG, total): the chain
// that starts at a leaves the segment at e + map[a] (BG_FAR: further than 16 bits say; BG_BAD: it does not leave it).
__global__ void __launch_bounds__(64) k_bg_chain(const uint8_t *__restrict__ data, long long total, uint16_t *map) {
    const int lane = threadIdx.x;
    const long long base = (long long)blockIdx.x * BG_SEG;
    const long long seg_end = min(base + BG_SEG, total);
    const int n = (int)(seg_end - base);
    for (int c = (n + BG_STEP - 1) / BG_STEP - 1; c >= 0; --c) {
        const int o = c * BG_STEP + lane;
        if (lane < BG_STEP && o < n) {
            const long long a = base + o;
            unsigned v = BG_BAD;
            if (a + 4 <= total) {
                const int bs = (int)bg_ld32(data + a);
                if (bs >= 32) {
                    const long long next = a + 4 + bs;      // >= a + 36: an offset of a step done before this one
                    if (next >= seg_end) v = next - seg_end < (long long)BG_FAR ? (unsigned)(next - seg_end) : BG_FAR;
                    else v = map[next];
                }
            }
            map[a] = (uint16_t)v;
        }
        wc_sync();                                  // this step's stores, before the next step's loads
    }
}

// entry[s]: the offset inside segment s at which the real chain enters it, -1 where it does not (a record covers the
// whole segment, or the chain has ended).  One wave, every lane with the same values.
__global__ void __launch_bounds__(64) k_bg_link(const uint8_t *__restrict__ data, long long total, long long first,
                                                const uint16_t *__restrict__ map, int n_seg, int *entry) {
    const int lane = threadIdx.x;
    for (int s = lane; s < n_seg; s += 64) entry[s] = -1;
    wc_sync();
    long long a = first;
    while (a < total) {                             // a moves to the end of its segment or beyond in every pass
        const long long s = a / BG_SEG, seg_end = min((s + 1) * BG_SEG, total);
        if (lane == 0) entry[s] = (int)(a - s * BG_SEG);
        const unsigned v = map[a];
        if (v == BG_BAD) break;
        if (v != BG_FAR) { a = seg_end + v; continue; }
        long long b = a;
        while (b < seg_end) {                       // b grows by 36 or more
            if (b + 4 > total) break;
            const int bs = (int)bg_ld32(data + b);
            if (bs < 32) break;
            b += 4 + (long long)bs;
        }
        if (b < seg_end) break;                     // (not reached: BG_FAR says that the chain leaves the segment)
        a = b;
    }
}

__global__ void __launch_bounds__(64) k_bg_begin(unsigned long long *m, long long total) {
    if (threadIdx.x == 0) {
        m[BG_PLACED] = 0;
        m[BG_TAIL] = (unsigned long long)total;
    }
}

// The walk of `total` bytes (a whole file, or carry + chunk), the first of them at the file's inflated offset abs_base.
// A record that overruns `total`, its block_size word included, is the truncation error only where the file ends with
// these bytes (`last`); before that it is where the next carry starts: its offset goes to m[BG_TAIL] (one lane at most
// meets it: the chain is one) and the walk stops there.  <true> appends at m[BG_BASE]; refs[] holds the placed records
// of these bytes alone.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_bg_walk(const uint8_t *__restrict__ data, long long total, long long abs_base, int last,
                                                 int n_ref, const int *__restrict__ entry, int n_seg, int *__restrict__ cnt,
                                                 const long long *__restrict__ seg_base, unsigned long long *m,
                                                 int32_t *__restrict__ pos, uint8_t *__restrict__ mapq,
                                                 uint16_t *__restrict__ flag, int32_t *__restrict__ mate, int32_t *__restrict__ refs) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_seg) return;
    const int e = entry[t];
    if (e < 0) {
        if (!WRITE) cnt[t] = 0;
        return;
    }
    long long a = (long long)t * BG_SEG + e;
    const long long seg_end = min((long long)(t + 1) * BG_SEG, total);
    long long local = WRITE ? seg_base[t] : 0;
    const long long out_base = WRITE ? (long long)m[BG_BASE] : 0;
    unsigned long long mapped = 0, unmapped = 0, nocoord = 0;
    int placed = 0;
    while (a < seg_end) {                           // a grows by 36 or more
        wc::BamRecord rec;
        const int bad = wc::bam_record(data + a, total - a, n_ref, rec);
        if (bad == wc::BAM_R_TRUNC && !last) {
            if (!WRITE) m[BG_TAIL] = (unsigned long long)a;
            break;
        }
        if (bad != wc::BAM_R_OK) {
            if (!WRITE) atomicMin(&m[BG_RECERR], ((unsigned long long)(abs_base + a) << 3) | (unsigned)bad);
            break;
        }
        if (rec.flag & 4u) ++unmapped;
        if (rec.ref < 0) {
            ++nocoord;
        } else {
            if (!(rec.flag & 4u)) ++mapped;
            if (WRITE) {
                const long long idx = out_base + local;
                pos[idx] = rec.pos;
                mapq[idx] = rec.mapq;
                flag[idx] = (uint16_t)rec.flag;
                mate[idx] = rec.mate_pos;
                refs[local] = rec.ref;
            }
            ++local;
            ++placed;
        }
        a += 4 + (long long)rec.block_size;
    }
    if (!WRITE) {
        cnt[t] = placed;
        if (mapped) atomicAdd(&m[0], mapped);
        if (unmapped) atomicAdd(&m[1], unmapped);
        if (nocoord) atomicAdd(&m[2], nocoord);
    }
}

// exclusive sums of cnt[0 .. n) into base[], the total into *sum; one workgroup
__global__ void __launch_bounds__(256) k_bg_scan(const int *__restrict__ cnt, int n, long long *__restrict__ base,
                                                 unsigned long long *sum) {
    __shared__ long long part[256];
    const int t = threadIdx.x, chunk = (n + 255) / 256;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    long long s = 0;
    for (int i = lo; i < hi; ++i) s += cnt[i];
    part[t] = s;
    wc_sync();
    if (t == 0) {
        long long run = 0;
        for (int i = 0; i < 256; ++i) {
            const long long v = part[i];
            part[i] = run;
            run += v;
        }
        *sum = (unsigned long long)run;
    }
    wc_sync();
    s = part[t];
    for (int i = lo; i < hi; ++i) {
        base[i] = s;
        s += cnt[i];
    }
}

// The order check on the placed records of these bytes: m[BG_ORDERR] is the least (placed index in the file << 2 | kind)
// with kind 1 a lower reference than the record before, 2 a lower position.  The predecessor of the first is the last
// placed record of the chunks before (its reference in m[BG_LASTREF], its position in the output).  The grid covers
// m[BG_PLACED] records or more.
__global__ void __launch_bounds__(256) k_bg_order(const int32_t *__restrict__ refs, const int32_t *__restrict__ pos,
                                                  unsigned long long *m) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)m[BG_PLACED]) return;
    const long long base = (long long)m[BG_BASE], g = base + i;
    if (g == 0) return;
    const int a = i ? refs[i - 1] : (int)(long long)m[BG_LASTREF], b = refs[i];
    const unsigned kind = b < a ? 1u : (b == a && pos[g] < pos[g - 1]) ? 2u : 0u;
    if (kind) atomicMin(&m[BG_ORDERR], ((unsigned long long)g << 2) | kind);
}

// acc[r] += the number of these bytes' placed records of references below r (refs[] ascends, or the order check fails):
// behind the last chunk acc[r] is the number of the file's placed records of references below r
__global__ void __launch_bounds__(256) k_bg_offsets(const int32_t *__restrict__ refs, const unsigned long long *__restrict__ m,
                                                    int n_ref, long long *__restrict__ acc) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r > n_ref) return;
    long long lo = 0, hi = (long long)m[BG_PLACED];
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (refs[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    acc[r] += lo;
}

__global__ void __launch_bounds__(64) k_bg_advance(const int32_t *__restrict__ refs, unsigned long long *m) {
    if (threadIdx.x) return;
    const long long n = (long long)m[BG_PLACED];
    if (n) {
        m[BG_LASTREF] = (unsigned long long)(long long)refs[n - 1];
        m[BG_BASE] += (unsigned long long)n;
    }
}

// ---- the bounded route (wc_convert_bam_stream_dev): a chunk's placed records go to a buffer of the chunk's own, records
// from element 1 on; element 0 of the positions keeps the last position of the chunks before for the order check
__global__ void __launch_bounds__(64) k_bg_keep_last(int32_t *pos_buf, const unsigned long long *__restrict__ m) {
    if (threadIdx.x) return;
    const long long n = (long long)m[BG_PLACED];
    if (n) pos_buf[0] = pos_buf[n];
}

// The slice table of the chunk for the picked references picked[n_chrom] (ascending): so[c] = the chunk's placed records
// of picked references in front of picked[c], from[c] = the chunk's placed records of references below picked[c].
// refs[] ascends (the order check has passed).  One workgroup, n_chrom <= 256.
__global__ void __launch_bounds__(256) k_bg_slice(const int32_t *__restrict__ refs, const unsigned long long *__restrict__ m,
                                                  const int32_t *__restrict__ picked, int n_chrom, int *__restrict__ so,
                                                  int *__restrict__ from) {
    __shared__ int s_cnt[256];
    const int c = (int)threadIdx.x;
    const long long n = (long long)m[BG_PLACED];
    int here = 0;
    if (c < n_chrom) {
        const int r = picked[c];
        long long lo = 0, hi = n;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (refs[mid] < r) lo = mid + 1;
            else hi = mid;
        }
        const long long begin = lo;
        hi = n;
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (refs[mid] <= r) lo = mid + 1;
            else hi = mid;
        }
        from[c] = (int)begin;
        here = (int)(lo - begin);
    }
    s_cnt[c] = here;
    wc_sync();
    if (c == 0) {
        int run = 0;
        for (int k = 0; k < n_chrom; ++k) {
            so[k] = run;
            run += s_cnt[k];
        }
        so[n_chrom] = run;
    }
}

// the chunk's records of the picked references side by side: record i of picked[c] goes to so[c] + (i - from[c])
__global__ void __launch_bounds__(256) k_bg_gather(const int32_t *__restrict__ refs, const unsigned long long *__restrict__ m,
                                                   const int32_t *__restrict__ picked, int n_chrom, const int *__restrict__ so,
                                                   const int *__restrict__ from, const int32_t *__restrict__ pos,
                                                   const uint8_t *__restrict__ mapq, const uint16_t *__restrict__ flag,
                                                   const int32_t *__restrict__ mate, int32_t *__restrict__ pos_out,
                                                   uint8_t *__restrict__ mapq_out, uint16_t *__restrict__ flag_out,
                                                   int32_t *__restrict__ mate_out) {
    __shared__ int s_picked[256], s_so[256], s_from[256];
    if ((int)threadIdx.x < n_chrom) {
        s_picked[threadIdx.x] = picked[threadIdx.x];
        s_so[threadIdx.x] = so[threadIdx.x];
        s_from[threadIdx.x] = from[threadIdx.x];
    }
    wc_sync();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)m[BG_PLACED]) return;
    const int r = refs[i];
    int lo = 0, hi = n_chrom;                           // the first picked reference that is not below r
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_picked[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= n_chrom || s_picked[lo] != r) return;     // a reference the conversion skips
    const long long d = (long long)s_so[lo] + (i - (long long)s_from[lo]);
    pos_out[d] = pos[i];
    mapq_out[d] = mapq[i];
    flag_out[d] = flag[i];
    mate_out[d] = mate[i];
}

struct DevMem {             // a device allocation of one call
    void *p = nullptr;
    DevMem() = default;
    DevMem(const DevMem &) = delete;
    DevMem &operator=(const DevMem &) = delete;
    ~DevMem() { release(); }
    int alloc(size_t bytes) {
        hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
        if (e != hipSuccess) {
            p = nullptr;
            wc::set_error("hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
            return WC_E_HIP;
        }
        return WC_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    void *take() {
        void *q = p;
        p = nullptr;
        return q;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct Events {
    hipEvent_t ev[9] = {nullptr};
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

int first_bad_block(const std::vector<int> &status) {
    for (size_t k = 0; k < status.size(); ++k)
        if (status[k]) return (int)k;
    return -1;
}

// One walk: `total` inflated bytes at `data` (a whole file, or carry + chunk), the first of them at the file's inflated
// offset abs_base, the records from offset `first`; `last`: the file ends with them.  The working arrays hold n_seg
// segments, m the BG_WORDS device words.
struct Walk {
    const uint8_t *data;
    long long total, abs_base, first;
    int last, n_ref, n_seg;
    uint16_t *map;
    int *entry, *cnt;
    long long *seg_base;
    unsigned long long *m;
};

// chain -> link -> count -> scan: behind them m[BG_PLACED], m[BG_RECERR], m[BG_TAIL] and the counters are these bytes'.
// ev (optional): three events, recorded behind the chain maps, the link, and the count with its scan.
int launch_count(hipStream_t stream, const Walk &w, hipEvent_t *ev) {
    hipLaunchKernelGGL(k_bg_chain, dim3((unsigned)w.n_seg), dim3(64), 0, stream, w.data, w.total, w.map);
    if (ev) WC_HIP(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(k_bg_link, dim3(1), dim3(64), 0, stream, w.data, w.total, w.first, (const uint16_t *)w.map, w.n_seg, w.entry);
    if (ev) WC_HIP(hipEventRecord(ev[1], stream));
    hipLaunchKernelGGL(k_bg_walk<false>, dim3((unsigned)((w.n_seg + 255) / 256)), dim3(256), 0, stream, w.data, w.total, w.abs_base,
                       w.last, w.n_ref, (const int *)w.entry, w.n_seg, w.cnt, (const long long *)nullptr, w.m, (int32_t *)nullptr,
                       (uint8_t *)nullptr, (uint16_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr);
    hipLaunchKernelGGL(k_bg_scan, dim3(1), dim3(256), 0, stream, (const int *)w.cnt, w.n_seg, w.seg_base, w.m + BG_PLACED);
    if (ev) WC_HIP(hipEventRecord(ev[2], stream));
    return WC_OK;
}

// fields -> order -> offsets, behind launch_count: the placed records' fields appended to the four arrays at m[BG_BASE],
// their references to refs[] (from 0), the order check, acc[] advanced.  order_room: m[BG_PLACED] or any number above it.
// ev (optional): two events, recorded behind the fields, and the order check with the offsets.
int launch_fields(hipStream_t stream, const Walk &w, int32_t *pos, uint8_t *mapq, uint16_t *flag, int32_t *mate, int32_t *refs,
                  long long *acc, long long order_room, hipEvent_t *ev) {
    hipLaunchKernelGGL(k_bg_walk<true>, dim3((unsigned)((w.n_seg + 255) / 256)), dim3(256), 0, stream, w.data, w.total, w.abs_base,
                       w.last, w.n_ref, (const int *)w.entry, w.n_seg, (int *)nullptr, (const long long *)w.seg_base, w.m, pos, mapq,
                       flag, mate, refs);
    if (ev) WC_HIP(hipEventRecord(ev[0], stream));
    hipLaunchKernelGGL(k_bg_order, dim3((unsigned)((order_room + 255) / 256)), dim3(256), 0, stream, (const int32_t *)refs,
                       (const int32_t *)pos, w.m);
    hipLaunchKernelGGL(k_bg_offsets, dim3((unsigned)(w.n_ref / 256 + 1)), dim3(256), 0, stream, (const int32_t *)refs,
                       (const unsigned long long *)w.m, w.n_ref, acc);
    if (ev) WC_HIP(hipEventRecord(ev[1], stream));
    return WC_OK;
}

// What one status read says, the first kind of defect first: a damaged block (st: the statuses of the blocks from the
// file's block first_block on), a record defect, an order defect.  got: the BG_WORDS device words; data_end: the file's
// inflated offset behind the bytes walked.  For the pair of an order defect: refs (device) holds the references of the
// placed records from the file's index placed_before on, prev_last_ref that of the one before them, pos (device) the
// positions of all.  WC_OK where nothing is wrong.
int check_status(const unsigned long long *got, const std::vector<int> &st, long long first_block, long long data_end, int n_ref,
                 const int32_t *refs, const int32_t *pos, long long placed_before, long long prev_last_ref) {
    const int bad = first_bad_block(st);
    WC_CHECK(bad < 0, WC_E_FORMAT, "bam: damaged BGZF block %lld (%s)", first_block + bad,
             st[(size_t)(bad < 0 ? 0 : bad)] == BG_E_CRC ? "CRC failed" : "inflate failed");
    if (got[BG_RECERR] != ~0ull) {
        const long long at = (long long)(got[BG_RECERR] >> 3);
        switch ((int)(got[BG_RECERR] & 7u)) {
            case wc::BAM_R_BS: wc::set_error("bam: the record at inflated offset %lld has a block_size below its 32 fixed bytes", at); break;
            case wc::BAM_R_FIELDS: wc::set_error("bam: the fields of the record at inflated offset %lld overrun its block_size", at); break;
            case wc::BAM_R_REF: wc::set_error("bam: the record at inflated offset %lld names a reference beyond the %d of the header", at, n_ref); break;
            default: wc::set_error("bam: truncated: the record at inflated offset %lld overruns the data (%lld bytes)", at, data_end);
        }
        return WC_E_FORMAT;
    }
    if (got[BG_ORDERR] != ~0ull) {
        const long long g = (long long)(got[BG_ORDERR] >> 2), local = g - placed_before;
        int32_t two_ref[2] = {(int32_t)prev_last_ref, 0}, two_pos[2] = {0, 0};
        if (local > 0) WC_HIP(hipMemcpy(two_ref, refs + local - 1, 8, hipMemcpyDeviceToHost));
        else WC_HIP(hipMemcpy(two_ref + 1, refs, 4, hipMemcpyDeviceToHost));
        WC_HIP(hipMemcpy(two_pos, pos + g - 1, 8, hipMemcpyDeviceToHost));
        if ((got[BG_ORDERR] & 3u) == 1u)
            wc::set_error("bam: not coordinate-sorted: placed record %lld of reference %d follows reference %d (the records of a "
                          "reference must be contiguous, references in header order)", g, two_ref[1], two_ref[0]);
        else
            wc::set_error("bam: not coordinate-sorted: position %d follows %d in reference %d (placed record %lld)", two_pos[1],
                          two_pos[0], two_ref[1], g);
        return WC_E_ARG;
    }
    return WC_OK;
}

}  // namespace

struct wc_bam_dev {
    std::vector<std::string> names;
    std::vector<int64_t> lengths, offsets;
    void *pos = nullptr, *mapq = nullptr, *flag = nullptr, *mate = nullptr;
    int64_t n = 0, mapped = 0, unmapped = 0, no_coordinate = 0, name_bytes = 0, need = 0, budget = 0;
    double times[8] = {0};
    int64_t stream_info[8] = {0};       // wc_bam_dev_stream_info (a streamed open)
    ~wc_bam_dev() {
        for (void *p : {pos, mapq, flag, mate})
            if (p) (void)hipFree(p);
    }
};

namespace {

int open_dev(wc_ctx *ctx, hipStream_t stream, const wc_bamfile &f, int64_t budget, wc_bam_dev &h) {
    const auto began = std::chrono::steady_clock::now();
    h.names = f.names;
    h.lengths = f.lengths;
    h.name_bytes = f.name_bytes;
    const int n_ref = (int)f.names.size();
    h.offsets.assign((size_t)n_ref + 1, 0);
    const int64_t total = f.total, n_blocks = (int64_t)f.blocks.size();
    const int64_t n_seg = (total + BG_SEG - 1) / BG_SEG;
    // the need, from the directory alone: compressed bytes, directory and status, the inflated bytes, the map (2 bytes per
    // inflated byte), three words per segment, and the output of the most records the data can hold (36 bytes each;
    // 15 bytes of fields per placed record, the reference numbers included)
    const int64_t max_rec = total / BG_STEP + 1;
    const int64_t need = (int64_t)f.size + WC_BGZF_PAD + n_blocks * (int64_t)(sizeof(wc::BgzfBlock) + 4) + total + 64 +
                         2 * n_seg * BG_SEG + 16 * n_seg + 15 * max_rec + 8 * ((int64_t)n_ref + 1) + 4096;
    if (budget <= 0) {
        size_t free_b = 0, total_b = 0;
        WC_HIP(hipMemGetInfo(&free_b, &total_b));
        budget = (int64_t)(BG_BUDGET_FRACTION * (double)free_b);
    }
    h.need = need;
    h.budget = budget;
    WC_CHECK(need <= budget, WC_E_LIMIT, "bam: the device reader needs %lld bytes, budget %lld", (long long)need, (long long)budget);
    WC_CHECK(n_seg < (int64_t)INT_MAX / 2 && n_blocks < (int64_t)INT_MAX, WC_E_LIMIT, "bam: %lld inflated bytes in one call",
             (long long)total);
    Events E;
    for (hipEvent_t &e : E.ev) WC_HIP(hipEventCreate(&e));
    DevMem comp, dir, status, plain, map, entry, cnt, base, misc;
    int rc;
    if ((rc = comp.alloc(f.size + WC_BGZF_PAD)) || (rc = dir.alloc(sizeof(wc::BgzfBlock) * (size_t)n_blocks)) ||
        (rc = status.alloc(4 * (size_t)n_blocks)) || (rc = plain.alloc((size_t)total + 64)) ||
        (rc = map.alloc(2 * (size_t)n_seg * BG_SEG)) || (rc = entry.alloc(4 * (size_t)n_seg)) ||
        (rc = cnt.alloc(4 * (size_t)n_seg)) || (rc = base.alloc(8 * (size_t)n_seg)) || (rc = misc.alloc(8 * BG_WORDS)))
        return rc;
    // to the walk the file is one chunk, the last, with nothing before it
    unsigned long long *m = misc.as<unsigned long long>();
    unsigned long long got[BG_WORDS] = {0};
    got[BG_RECERR] = got[BG_ORDERR] = ~0ull;
    got[BG_LASTREF] = (unsigned long long)-1ll;
    const Walk walk = {plain.as<uint8_t>(), (long long)total, 0, (long long)f.first_record, 1, n_ref, (int)n_seg,
                       map.as<uint16_t>(), entry.as<int>(), cnt.as<int>(), base.as<long long>(), m};
    WC_HIP(hipEventRecord(E.ev[0], stream));
    WC_HIP(hipMemcpyAsync(m, got, sizeof(got), hipMemcpyHostToDevice, stream));
    WC_HIP(hipMemcpyAsync(comp.p, f.data, f.size + WC_BGZF_PAD, hipMemcpyHostToDevice, stream));
    if (n_blocks) WC_HIP(hipMemcpyAsync(dir.p, f.blocks.data(), sizeof(wc::BgzfBlock) * (size_t)n_blocks, hipMemcpyHostToDevice, stream));
    WC_HIP(hipEventRecord(E.ev[1], stream));
    if (n_blocks)
        hipLaunchKernelGGL(k_bg_inflate, dim3((unsigned)n_blocks), dim3(64), 0, stream, (const uint8_t *)comp.as<uint8_t>(),
                           (const wc::BgzfBlock *)dir.as<wc::BgzfBlock>(), plain.as<uint8_t>(), status.as<int>());
    WC_HIP(hipEventRecord(E.ev[2], stream));
    if ((rc = launch_count(stream, walk, E.ev + 3))) return rc;     // n_seg >= 1: the header lies in the data
    WC_HIP(hipGetLastError());
    std::vector<int> st((size_t)n_blocks, 0);
    if (n_blocks) WC_HIP(hipMemcpyAsync(st.data(), status.p, 4 * (size_t)n_blocks, hipMemcpyDeviceToHost, stream));
    WC_HIP(hipMemcpyAsync(got, m, sizeof(got), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    // every block and record defect here, before the arrays are sized and any order is looked at
    if ((rc = check_status(got, st, 0, total, n_ref, nullptr, nullptr, 0, -1))) return rc;
    comp.release();
    map.release();
    const unsigned long long n = got[BG_PLACED];
    WC_CHECK(n <= (unsigned long long)INT32_MAX, WC_E_LIMIT, "bam: more than 2^31 - 1 placed records");
    h.mapped = (int64_t)got[0];
    h.unmapped = (int64_t)got[1];
    h.no_coordinate = (int64_t)got[2];
    h.n = (int64_t)n;
    DevMem pos, mapq, flag, mate, refs, offs;
    if ((rc = pos.alloc(4 * (size_t)n)) || (rc = mapq.alloc((size_t)n)) || (rc = flag.alloc(2 * (size_t)n)) ||
        (rc = mate.alloc(4 * (size_t)n)) || (rc = refs.alloc(4 * (size_t)n)) || (rc = offs.alloc(8 * ((size_t)n_ref + 1))))
        return rc;
    WC_HIP(hipMemsetAsync(offs.p, 0, 8 * ((size_t)n_ref + 1), stream));
    WC_HIP(hipEventRecord(E.ev[6], stream));
    // the order grid by n, which the host knows here (a file without placed records: one workgroup that finds none)
    if ((rc = launch_fields(stream, walk, pos.as<int32_t>(), mapq.as<uint8_t>(), flag.as<uint16_t>(), mate.as<int32_t>(),
                            refs.as<int32_t>(), offs.as<long long>(), std::max<long long>((long long)n, 1), E.ev + 7)))
        return rc;
    WC_HIP(hipGetLastError());
    WC_HIP(hipMemcpyAsync(got, m, sizeof(got), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipMemcpyAsync(h.offsets.data(), offs.p, 8 * ((size_t)n_ref + 1), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    if ((rc = check_status(got, st, 0, total, n_ref, refs.as<int32_t>(), pos.as<int32_t>(), 0, -1))) return rc;
    static const int pairs[7][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {4, 5}, {6, 7}, {7, 8}};
    for (int k = 0; k < 7; ++k) {
        float ms = 0.f;
        WC_HIP(hipEventElapsedTime(&ms, E.ev[pairs[k][0]], E.ev[pairs[k][1]]));
        h.times[k] = ms;
    }
    h.times[7] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - began).count();
    h.pos = pos.take();
    h.mapq = mapq.take();
    h.flag = flag.take();
    h.mate = mate.take();
    return WC_OK;
}

// ---- the streamed open ------------------------------------------------------------------------------------------------
struct ChunkCloser {
    wc_bamchunks *it = nullptr;
    ~ChunkCloser() { wc_bamchunks_close(it); }
};
struct CopyStream {
    hipStream_t s = nullptr;
    hipEvent_t done[2] = {nullptr, nullptr};
    ~CopyStream() {
        if (s) (void)hipStreamSynchronize(s);           // no copy may outlive the staging buffers
        for (hipEvent_t e : done)
            if (e) (void)hipEventDestroy(e);
        if (s) (void)hipStreamDestroy(s);
    }
};
struct Sized {              // a working buffer that grows to the largest need seen (its old content is not kept)
    DevMem mem;
    size_t cap = 0;
    int reserve(size_t want) {
        if (want <= cap) return WC_OK;
        mem.release();
        cap = 0;
        const int rc = mem.alloc(want);
        if (rc == WC_OK) cap = want;
        return rc;
    }
};

// The sink of the bounded route: every chunk's records are fed to `run` (the references picked[n_chrom] of the file,
// ascending) and dropped; no arrays are kept.
struct Bounded {
    wc_convert_run *run = nullptr;
    const int32_t *picked = nullptr;
    int n_chrom = 0;
    bool paired = false;
    int64_t peak_all = 0;           // peak device bytes, everything
};

int stream_dev(wc_ctx *ctx, hipStream_t stream, const char *path, int64_t chunk_bytes, wc_bam_dev &h, Bounded *bd = nullptr) {
    const auto began = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    ChunkCloser chunks;
    int rc = wc_bamchunks_open(path, ctx->device, chunk_bytes, &chunks.it);
    if (rc) return rc;
    const wc_bamfile &hdr = wc::bamchunks_header(chunks.it);
    h.names = hdr.names;
    h.lengths = hdr.lengths;
    h.name_bytes = hdr.name_bytes;
    const int n_ref = (int)hdr.names.size();
    h.offsets.assign((size_t)n_ref + 1, 0);
    const long long first_record = hdr.first_record;

    CopyStream copy;
    WC_HIP(hipStreamCreateWithFlags(&copy.s, hipStreamNonBlocking));
    for (hipEvent_t &e : copy.done) WC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    // comp, dir: one per chunk in flight (the copy of chunk i + 1 runs beside the decode of chunk i); plain: the carry
    // moves from one to the other
    Sized comp[2], dir[2], plain[2], status, map, entry, cnt, base, refs;
    Sized rec[4], gat[4];                               // bounded route: the chunk's records, and those of the picked references
    DevMem acc, misc, out[4], pick;                     // pick: picked[], so[], from[] of the bounded route
    static const size_t width[4] = {4, 1, 2, 4};        // pos, mapq, flag, mate_pos
    int64_t out_cap = 0, peak_work = 0, peak_all = 0, regrows = 0, run_bytes = 0;
    auto account = [&]() {
        int64_t w = 8 * ((int64_t)n_ref + 1) + 8 * BG_WORDS;
        for (const Sized *b : {&comp[0], &comp[1], &dir[0], &dir[1], &plain[0], &plain[1], &status, &map, &entry, &cnt, &base, &refs})
            w += (int64_t)b->cap;
        peak_work = std::max(peak_work, w);
        peak_all = std::max(peak_all, w + 11 * out_cap);
        if (bd) {
            for (int k = 0; k < 4; ++k) w += (int64_t)(rec[k].cap + gat[k].cap);
            bd->peak_all = std::max(bd->peak_all, w + run_bytes + 12 * ((int64_t)bd->n_chrom + 1));
        }
    };
    if (bd) {
        for (int c = 0; c < bd->n_chrom; ++c)
            WC_CHECK(bd->picked[c] >= 0 && bd->picked[c] < n_ref && (!c || bd->picked[c] > bd->picked[c - 1]), WC_E_ARG,
                     "convert: reference %d of %d (the picked references ascend)", bd->picked[c], n_ref);
        if ((rc = pick.alloc(12 * ((size_t)bd->n_chrom + 1)))) return rc;
        WC_HIP(hipMemcpyAsync(pick.p, bd->picked, 4 * (size_t)bd->n_chrom, hipMemcpyHostToDevice, stream));
        int64_t info[8];
        if ((rc = wc_convert_run_info(bd->run, info))) return rc;
        run_bytes = info[1];
    }
    const int32_t *picked_dev = pick.as<int32_t>();
    int *so_dev = bd ? pick.as<int>() + bd->n_chrom + 1 : nullptr, *from_dev = bd ? so_dev + bd->n_chrom + 1 : nullptr;
    if ((rc = acc.alloc(8 * ((size_t)n_ref + 1))) || (rc = misc.alloc(8 * BG_WORDS))) return rc;
    unsigned long long *m = misc.as<unsigned long long>();
    unsigned long long got[BG_WORDS] = {0};
    got[BG_RECERR] = got[BG_ORDERR] = ~0ull;
    got[BG_LASTREF] = (unsigned long long)-1ll;
    WC_HIP(hipMemcpyAsync(m, got, sizeof(got), hipMemcpyHostToDevice, stream));
    WC_HIP(hipMemsetAsync(acc.p, 0, 8 * ((size_t)n_ref + 1), stream));

    double wait_reader = 0., wait_device = 0.;
    auto next_chunk = [&](wc_bamchunk &c) {
        const auto t0 = std::chrono::steady_clock::now();
        const int r = wc::bamchunks_next(chunks.it, c);
        wait_reader += ms_since(t0);
        return r;
    };
    auto upload = [&](const wc_bamchunk &c, int slot) {
        int r;
        if ((r = comp[slot].reserve((size_t)c.bytes + WC_BGZF_PAD)) || (r = dir[slot].reserve(sizeof(wc::BgzfBlock) * (size_t)c.n_blocks)))
            return r;
        account();
        WC_HIP(hipMemcpyAsync(comp[slot].mem.p, c.data, (size_t)c.bytes + WC_BGZF_PAD, hipMemcpyHostToDevice, copy.s));
        WC_HIP(hipMemcpyAsync(dir[slot].mem.p, c.blocks, sizeof(wc::BgzfBlock) * (size_t)c.n_blocks, hipMemcpyHostToDevice, copy.s));
        WC_HIP(hipEventRecord(copy.done[slot], copy.s));
        return (int)WC_OK;
    };

    wc_bamchunk cur, nxt;
    if ((rc = next_chunk(cur))) return rc;
    if (cur.data && (rc = upload(cur, 0))) return rc;
    long long carry = 0, tail = 0, abs_next = 0, placed = 0, prev_last_ref = -1;
    int64_t n_chunks = 0, max_comp = 0, max_infl = 0, max_carry = 0;
    std::vector<int> st;
    for (int64_t i = 0; cur.data; ++i) {
        const int s = (int)(i & 1);
        const long long total = carry + cur.inflated, abs_base = abs_next - carry;
        const int64_t n_seg = (total + BG_SEG - 1) / BG_SEG, n_blocks = cur.n_blocks;
        const int64_t max_rec = total / BG_STEP + 1;
        WC_CHECK(n_seg < (int64_t)INT_MAX / 2 && n_blocks < (int64_t)INT_MAX, WC_E_LIMIT, "bam: %lld inflated bytes in one chunk",
                 (long long)total);
        if ((rc = plain[s].reserve((size_t)n_seg * BG_SEG + 64)) || (rc = map.reserve(2 * (size_t)n_seg * BG_SEG)) ||
            (rc = entry.reserve(4 * (size_t)n_seg)) || (rc = cnt.reserve(4 * (size_t)n_seg)) || (rc = base.reserve(8 * (size_t)n_seg)) ||
            (rc = refs.reserve(4 * (size_t)((n_seg * BG_SEG) / BG_STEP + 1))) || (rc = status.reserve(4 * (size_t)n_blocks)))
            return rc;
        if (bd) {                                       // room for the most records this chunk can hold, behind element 0
            const size_t room = (size_t)max_rec + 1;
            if (4 * room > rec[0].cap && rec[0].cap) {  // the positions grow: element 0 moves along
                int32_t lead = 0;
                WC_HIP(hipStreamSynchronize(stream));
                WC_HIP(hipMemcpy(&lead, rec[0].mem.p, 4, hipMemcpyDeviceToHost));
                if ((rc = rec[0].reserve(4 * room))) return rc;
                WC_HIP(hipMemcpy(rec[0].mem.p, &lead, 4, hipMemcpyHostToDevice));
            }
            for (int k = 0; k < 4; ++k)
                if ((rc = rec[k].reserve(width[k] * room)) || (rc = gat[k].reserve(width[k] * room))) return rc;
        } else if (placed + max_rec > out_cap) {        // the arrays: room for the most records this chunk can hold
            const int64_t want = std::max<int64_t>(placed + max_rec, 2 * out_cap);
            DevMem grown[4];
            for (int k = 0; k < 4; ++k)
                if ((rc = grown[k].alloc(width[k] * (size_t)want))) return rc;
            peak_all = std::max(peak_all, peak_work + 11 * (out_cap + want));
            for (int k = 0; k < 4 && placed; ++k)
                WC_HIP(hipMemcpyAsync(grown[k].p, out[k].p, width[k] * (size_t)placed, hipMemcpyDeviceToDevice, stream));
            WC_HIP(hipStreamSynchronize(stream));
            for (int k = 0; k < 4; ++k) {
                out[k].release();
                out[k].p = grown[k].take();
            }
            if (out_cap) ++regrows;
            out_cap = want;
        }
        account();
        uint8_t *data = plain[s].mem.as<uint8_t>();
        if (carry)
            WC_HIP(hipMemcpyAsync(data, plain[s ^ 1].mem.as<uint8_t>() + tail, (size_t)carry, hipMemcpyDeviceToDevice, stream));
        WC_HIP(hipStreamWaitEvent(stream, copy.done[s], 0));
        hipLaunchKernelGGL(k_bg_begin, dim3(1), dim3(64), 0, stream, m, total);
        if (n_blocks)
            hipLaunchKernelGGL(k_bg_inflate, dim3((unsigned)n_blocks), dim3(64), 0, stream, (const uint8_t *)comp[s].mem.as<uint8_t>(),
                               (const wc::BgzfBlock *)dir[s].mem.as<wc::BgzfBlock>(), data + carry, status.mem.as<int>());
        // where the walk writes: the growing arrays; bounded route: the chunk's buffers, addressed so that the file's
        // placed record number `placed` (the running base on the device) lands on element 1
        auto sink = [&](int k) -> void * {
            if (!bd) return out[k].p;
            return (void *)((uintptr_t)rec[k].mem.p + width[k] - width[k] * (size_t)placed);
        };
        // the records: from the carry's first byte, or from the end of the header in the chunk that holds it
        const long long first = std::max(first_record - abs_base, 0ll);
        if (first < total) {
            const Walk walk = {data, total, abs_base, first, cur.last ? 1 : 0, n_ref, (int)n_seg, map.mem.as<uint16_t>(),
                               entry.mem.as<int>(), cnt.mem.as<int>(), base.mem.as<long long>(), m};
            // no host synchronise between the two: the order grid covers the most records the chunk can hold
            if ((rc = launch_count(stream, walk, nullptr)) ||
                (rc = launch_fields(stream, walk, (int32_t *)sink(0), (uint8_t *)sink(1), (uint16_t *)sink(2), (int32_t *)sink(3),
                                    refs.mem.as<int32_t>(), acc.as<long long>(), (long long)max_rec, nullptr)))
                return rc;
            hipLaunchKernelGGL(k_bg_advance, dim3(1), dim3(64), 0, stream, (const int32_t *)refs.mem.as<int32_t>(), m);
        }
        WC_HIP(hipGetLastError());
        // the staging buffer of this chunk is free once its copy has run: the reader thread may fill it with chunk i + 2,
        // and the copy of chunk i + 1 runs beside this chunk's kernels
        const auto t0 = std::chrono::steady_clock::now();
        WC_HIP(hipEventSynchronize(copy.done[s]));
        wait_device += ms_since(t0);
        const long long first_block = cur.first_block;
        const bool was_last = cur.last;
        ++n_chunks;
        max_comp = std::max<int64_t>(max_comp, cur.bytes);
        max_infl = std::max<int64_t>(max_infl, cur.inflated);
        abs_next += cur.inflated;
        const int rc_next = next_chunk(nxt);            // a defect of the next chunk waits for this chunk's status: file order
        char next_error[1024];
        if (rc_next) snprintf(next_error, sizeof(next_error), "%s", wc_last_error());
        else if (nxt.data && (rc = upload(nxt, s ^ 1))) return rc;
        st.assign((size_t)n_blocks, 0);
        if (n_blocks) WC_HIP(hipMemcpyAsync(st.data(), status.mem.p, 4 * (size_t)n_blocks, hipMemcpyDeviceToHost, stream));
        WC_HIP(hipMemcpyAsync(got, m, sizeof(got), hipMemcpyDeviceToHost, stream));
        const auto t1 = std::chrono::steady_clock::now();
        WC_HIP(hipStreamSynchronize(stream));
        wait_device += ms_since(t1);
        if ((rc = check_status(got, st, first_block, abs_base + total, n_ref, refs.mem.as<int32_t>(), (const int32_t *)sink(0), placed,
                               prev_last_ref)))
            return rc;
        if (bd && got[BG_PLACED]) {                     // the chunk is sound: its picked records to the run, behind the walk
            const long long here = (long long)got[BG_PLACED];
            // (behind the status read: an order defect's text shows the position the check compared with)
            hipLaunchKernelGGL(k_bg_keep_last, dim3(1), dim3(64), 0, stream, rec[0].mem.as<int32_t>(), (const unsigned long long *)m);
            hipLaunchKernelGGL(k_bg_slice, dim3(1), dim3(256), 0, stream, (const int32_t *)refs.mem.as<int32_t>(),
                               (const unsigned long long *)m, picked_dev, bd->n_chrom, so_dev, from_dev);
            hipLaunchKernelGGL(k_bg_gather, dim3((unsigned)((here + 255) / 256)), dim3(256), 0, stream,
                               (const int32_t *)refs.mem.as<int32_t>(), (const unsigned long long *)m, picked_dev, bd->n_chrom,
                               (const int *)so_dev, (const int *)from_dev, (const int32_t *)rec[0].mem.as<int32_t>() + 1,
                               (const uint8_t *)rec[1].mem.as<uint8_t>() + 1, (const uint16_t *)rec[2].mem.as<uint16_t>() + 1,
                               (const int32_t *)rec[3].mem.as<int32_t>() + 1, gat[0].mem.as<int32_t>(), gat[1].mem.as<uint8_t>(),
                               gat[2].mem.as<uint16_t>(), gat[3].mem.as<int32_t>());
            WC_HIP(hipGetLastError());
            if ((rc = wc::convert_feed_table_dev(bd->run, stream, gat[0].mem.as<int32_t>(), gat[1].mem.as<uint8_t>(),
                                                 bd->paired ? gat[2].mem.as<uint16_t>() : nullptr,
                                                 bd->paired ? gat[3].mem.as<int32_t>() : nullptr, so_dev, here)))
                return rc;
            int64_t info[8];
            if ((rc = wc_convert_run_info(bd->run, info))) return rc;
            run_bytes = info[1];
            account();
        }
        placed = (long long)got[BG_BASE];
        WC_CHECK(bd || placed <= (long long)INT32_MAX, WC_E_LIMIT, "bam: more than 2^31 - 1 placed records");
        prev_last_ref = (long long)got[BG_LASTREF];
        tail = (long long)got[BG_TAIL];
        carry = was_last ? 0 : total - tail;
        max_carry = std::max<int64_t>(max_carry, carry);
        if (rc_next) {
            wc::set_error("%s", next_error);
            return rc_next;
        }
        cur = nxt;
    }
    h.mapped = (int64_t)got[0];
    h.unmapped = (int64_t)got[1];
    h.no_coordinate = (int64_t)got[2];
    h.n = placed;
    WC_HIP(hipMemcpyAsync(h.offsets.data(), acc.p, 8 * ((size_t)n_ref + 1), hipMemcpyDeviceToHost, stream));
    WC_HIP(hipStreamSynchronize(stream));
    h.need = peak_all;
    h.budget = 0;
    const int64_t info[8] = {n_chunks, max_comp, max_infl, max_carry, peak_work, wc::bamchunks_host_bytes(chunks.it), regrows,
                             wc::bamchunks_pinned(chunks.it) ? 1 : 0};
    for (int k = 0; k < 8; ++k) h.stream_info[k] = info[k];
    h.times[0] = wait_reader;
    h.times[1] = wait_device;
    h.times[7] = ms_since(began);
    h.pos = out[0].take();
    h.mapq = out[1].take();
    h.flag = out[2].take();
    h.mate = out[3].take();
    return WC_OK;
}

// a handle filled by `open` on the context's device, or none and open's code
template <class Open> int new_handle(wc_ctx *ctx, wc_bam_dev **out, Open open) {
    *out = nullptr;
    WC_HIP(hipSetDevice(ctx->device));
    wc_bam_dev *h = nullptr;
    int rc;
    try {
        h = new wc_bam_dev();
        rc = open(*h);
    } catch (const std::exception &e) {
        wc::set_error("bam: %s", e.what());
        rc = WC_E_LIMIT;
    }
    if (rc != WC_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_bam_chain_segment(void) { return BG_SEG; }

int wc_bam_open_dev(wc_ctx *ctx, void *stream, const wc_bamfile *file, int64_t budget_bytes, wc_bam_dev **out) {
    WC_CHECK(ctx && file && out, WC_E_ARG, "bam: NULL argument");
    return new_handle(ctx, out, [&](wc_bam_dev &h) { return open_dev(ctx, (hipStream_t)stream, *file, budget_bytes, h); });
}

int wc_bam_stream_dev(wc_ctx *ctx, void *stream, const char *path, int64_t chunk_bytes, wc_bam_dev **out) {
    WC_CHECK(ctx && path && out, WC_E_ARG, "bam: NULL argument");
    return new_handle(ctx, out, [&](wc_bam_dev &h) { return stream_dev(ctx, (hipStream_t)stream, path, chunk_bytes, h); });
}

int wc_bam_dev_stream_info(const wc_bam_dev *h, int64_t out[8]) {
    WC_CHECK(h && out, WC_E_ARG, "bam: NULL argument");
    for (int k = 0; k < 8; ++k) out[k] = h->stream_info[k];
    return WC_OK;
}

int wc_bam_dev_info(const wc_bam_dev *h, int64_t out[8]) {
    WC_CHECK(h && out, WC_E_ARG, "bam: NULL argument");
    out[0] = (int64_t)h->names.size();
    out[1] = h->n;
    out[2] = h->mapped;
    out[3] = h->unmapped;
    out[4] = h->no_coordinate;
    out[5] = h->name_bytes;
    out[6] = h->need;
    out[7] = h->budget;
    return WC_OK;
}

int wc_bam_dev_refs(const wc_bam_dev *h, char *names_out, int64_t names_cap, int64_t *lengths_out, int64_t *offsets_out) {
    WC_CHECK(h && names_out && lengths_out && offsets_out, WC_E_ARG, "bam: NULL argument");
    WC_CHECK(names_cap >= h->name_bytes, WC_E_ARG, "bam: %lld bytes of names, room for %lld", (long long)h->name_bytes,
             (long long)names_cap);
    char *w = names_out;
    for (size_t r = 0; r < h->names.size(); ++r) {
        memcpy(w, h->names[r].data(), h->names[r].size());
        w += h->names[r].size();
        *w++ = '\n';
        lengths_out[r] = h->lengths[r];
    }
    for (size_t r = 0; r < h->offsets.size(); ++r) offsets_out[r] = h->offsets[r];
    return WC_OK;
}

const int32_t *wc_bam_dev_pos(const wc_bam_dev *h) { return h ? (const int32_t *)h->pos : nullptr; }
const uint8_t *wc_bam_dev_mapq(const wc_bam_dev *h) { return h ? (const uint8_t *)h->mapq : nullptr; }
const uint16_t *wc_bam_dev_flag(const wc_bam_dev *h) { return h ? (const uint16_t *)h->flag : nullptr; }
const int32_t *wc_bam_dev_mate_pos(const wc_bam_dev *h) { return h ? (const int32_t *)h->mate : nullptr; }

int wc_bam_dev_times(const wc_bam_dev *h, double out[8]) {
    WC_CHECK(h && out, WC_E_ARG, "bam: NULL argument");
    for (int k = 0; k < 8; ++k) out[k] = h->times[k];
    return WC_OK;
}

int wc_bam_dev_fetch(const wc_bam_dev *h, int32_t *pos_out, uint8_t *mapq_out, uint16_t *flag_out, int32_t *mate_pos_out) {
    WC_CHECK(h, WC_E_ARG, "bam: NULL argument");
    const size_t n = (size_t)h->n;
    if (pos_out && n) WC_HIP(hipMemcpy(pos_out, h->pos, 4 * n, hipMemcpyDeviceToHost));
    if (mapq_out && n) WC_HIP(hipMemcpy(mapq_out, h->mapq, n, hipMemcpyDeviceToHost));
    if (flag_out && n) WC_HIP(hipMemcpy(flag_out, h->flag, 2 * n, hipMemcpyDeviceToHost));
    if (mate_pos_out && n) WC_HIP(hipMemcpy(mate_pos_out, h->mate, 4 * n, hipMemcpyDeviceToHost));
    return WC_OK;
}

void wc_bam_dev_close(wc_bam_dev *h) { delete h; }

int wc_bgzf_inflate(wc_ctx *ctx, const unsigned char *bgzf_bytes, int64_t n, unsigned char *out, int64_t cap, int64_t *out_len) {
    WC_CHECK(ctx && out_len && n >= 0 && cap >= 0 && (bgzf_bytes || n == 0) && (out || cap == 0), WC_E_ARG, "bgzf: unusable argument");
    *out_len = 0;
    std::vector<wc::BgzfBlock> blocks;
    int64_t total = 0;
    int rc = wc::bgzf_directory(bgzf_bytes, (size_t)n, blocks, total);
    if (rc) return rc;
    WC_CHECK(total <= cap, WC_E_ARG, "bgzf: %lld inflated bytes, room for %lld", (long long)total, (long long)cap);
    WC_CHECK(blocks.size() < (size_t)INT_MAX, WC_E_LIMIT, "bgzf: %zu blocks in one call", blocks.size());
    *out_len = total;
    if (blocks.empty()) return WC_OK;
    WC_HIP(hipSetDevice(ctx->device));
    DevMem comp, dir, status, plain;
    if ((rc = comp.alloc((size_t)n + WC_BGZF_PAD)) || (rc = dir.alloc(sizeof(wc::BgzfBlock) * blocks.size())) ||
        (rc = status.alloc(4 * blocks.size())) || (rc = plain.alloc((size_t)total + 64)))
        return rc;
    WC_HIP(hipMemset(comp.as<uint8_t>() + n, 0, WC_BGZF_PAD));
    WC_HIP(hipMemcpy(comp.p, bgzf_bytes, (size_t)n, hipMemcpyHostToDevice));
    WC_HIP(hipMemcpy(dir.p, blocks.data(), sizeof(wc::BgzfBlock) * blocks.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_bg_inflate, dim3((unsigned)blocks.size()), dim3(64), 0, (hipStream_t) nullptr,
                       (const uint8_t *)comp.as<uint8_t>(), (const wc::BgzfBlock *)dir.as<wc::BgzfBlock>(), plain.as<uint8_t>(),
                       status.as<int>());
    WC_HIP(hipGetLastError());
    std::vector<int> st(blocks.size(), 0);
    WC_HIP(hipMemcpy(st.data(), status.p, 4 * blocks.size(), hipMemcpyDeviceToHost));
    const int bad = first_bad_block(st);
    WC_CHECK(bad < 0, WC_E_FORMAT, "bgzf: damaged BGZF block %d (%s)", bad,
             st[(size_t)(bad < 0 ? 0 : bad)] == BG_E_CRC ? "CRC failed" : "inflate failed");
    if (total) WC_HIP(hipMemcpy(out, plain.p, (size_t)total, hipMemcpyDeviceToHost));
    return WC_OK;
}

int wc_convert_bam_stream_dev(wc_ctx *ctx, void *stream_, const char *path, int64_t chunk_bytes, const int32_t *refs, int n_chrom,
                              double binsize, int min_shift, int threshold, int min_mapq, int demand_pair,
                              const int64_t *bin_offsets, int32_t *counts_out, int64_t *stats_out, int64_t info_out[16]) {
    WC_CHECK(ctx && path && refs && bin_offsets && counts_out && stats_out && info_out, WC_E_ARG, "convert: NULL argument");
    WC_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    struct RunCloser {
        wc_convert_run *run = nullptr;
        ~RunCloser() { wc_convert_end(run); }
    } closer;
    int rc = wc_convert_begin(ctx, n_chrom, binsize, min_shift, threshold, min_mapq, demand_pair, bin_offsets, &closer.run);
    if (rc) return rc;
    Bounded bd;
    bd.run = closer.run;
    bd.picked = refs;
    bd.n_chrom = n_chrom;
    bd.paired = demand_pair != 0;
    wc_bam_dev h;                                       // the header and the counters only: it gets no arrays
    try {
        rc = stream_dev(ctx, stream, path, chunk_bytes, h, &bd);
    } catch (const std::exception &e) {
        wc::set_error("bam: %s", e.what());
        rc = WC_E_LIMIT;
    }
    if (rc) return rc;
    int64_t max_pending = 0;
    if ((rc = wc::convert_run_max_pending(closer.run, stream, &max_pending))) return rc;      // (waits for the last slice)
    if ((rc = wc_convert_finish(closer.run, counts_out, stats_out))) return rc;
    int64_t run_info[8];
    if ((rc = wc_convert_run_info(closer.run, run_info))) return rc;
    for (int k = 0; k < 16; ++k) info_out[k] = 0;
    info_out[0] = h.stream_info[0];                     // chunks
    info_out[1] = h.stream_info[1];                     // the largest chunk's compressed bytes
    info_out[2] = h.stream_info[3];                     // the largest byte carry
    info_out[3] = max_pending;                          // the largest run carry (positions)
    info_out[4] = bd.peak_all;                          // peak device bytes, everything
    info_out[5] = h.stream_info[5];                     // host staging bytes
    info_out[6] = h.n;                                  // placed records
    info_out[7] = h.stream_info[2];                     // the largest chunk's inflated bytes
    info_out[8] = h.mapped;
    info_out[9] = h.unmapped;
    info_out[10] = h.no_coordinate;
    info_out[11] = run_info[1];                         // of the peak: the run's own bytes (tables, kpos, counts, carry)
    return WC_OK;
}

int wc_convert_bam_dev(wc_ctx *ctx, void *stream_, const wc_bam_dev *h, const int32_t *refs, int n_chrom, double binsize,
                       int min_shift, int threshold, int min_mapq, int demand_pair, const int64_t *bin_offsets,
                       int32_t *counts_out, int64_t *stats_out) {
    WC_CHECK(ctx && h && refs && bin_offsets && counts_out && stats_out, WC_E_ARG, "convert: NULL argument");
    WC_CHECK(n_chrom >= 1 && n_chrom <= WC_CV_MAX_CHROM, WC_E_LIMIT, "convert: %d chromosomes (1..%d supported)", n_chrom,
             WC_CV_MAX_CHROM);
    const int64_t bins = bin_offsets[n_chrom];
    WC_CHECK(bins >= 0 && bins <= (int64_t)INT_MAX, WC_E_LIMIT, "convert: %lld bins in one call", (long long)bins);
    const int n_ref = (int)h->names.size();
    std::vector<int64_t> ro((size_t)n_chrom + 1, 0);
    bool contiguous = true;
    for (int c = 0; c < n_chrom; ++c) {
        WC_CHECK(refs[c] >= 0 && refs[c] < n_ref, WC_E_ARG, "convert: reference %d of %d", refs[c], n_ref);
        ro[(size_t)c + 1] = ro[(size_t)c] + h->offsets[(size_t)refs[c] + 1] - h->offsets[(size_t)refs[c]];
        if (c && h->offsets[(size_t)refs[c]] != h->offsets[(size_t)refs[c - 1] + 1]) contiguous = false;
    }
    const int64_t n = ro[(size_t)n_chrom];
    const bool paired = demand_pair != 0;
    WC_HIP(hipSetDevice(ctx->device));
    hipStream_t stream = (hipStream_t)stream_;
    int rc;
    if ((rc = ctx->tmp_c.reserve(sizeof(int32_t) * (size_t)(bins + 1) + 64))) return rc;
    int64_t *stats_dev = ctx->tmp_c.as<int64_t>();               // 8 words, then the counts
    const int64_t lo = h->offsets[(size_t)refs[0]];
    const int32_t *pos = (const int32_t *)h->pos + lo, *mate = (const int32_t *)h->mate + lo;
    const uint8_t *mapq = (const uint8_t *)h->mapq + lo;
    const uint16_t *flag = (const uint16_t *)h->flag + lo;
    if (!contiguous && n) {                                     // the picked references, gathered on the device
        if ((rc = ctx->tmp_a.reserve(4 * (size_t)n)) || (rc = ctx->tmp_b.reserve((size_t)n)) ||
            (paired && (rc = ctx->tmp_d.reserve(6 * (size_t)n + 8))))
            return rc;
        int32_t *mate_g = ctx->tmp_d.as<int32_t>();
        uint16_t *flag_g = paired ? reinterpret_cast<uint16_t *>(mate_g + n) : nullptr;
        for (int c = 0; c < n_chrom; ++c) {
            const int64_t from = h->offsets[(size_t)refs[c]], k = ro[(size_t)c + 1] - ro[(size_t)c], to = ro[(size_t)c];
            if (!k) continue;
            WC_HIP(hipMemcpyAsync(ctx->tmp_a.as<int32_t>() + to, (const int32_t *)h->pos + from, 4 * (size_t)k, hipMemcpyDeviceToDevice, stream));
            WC_HIP(hipMemcpyAsync(ctx->tmp_b.as<uint8_t>() + to, (const uint8_t *)h->mapq + from, (size_t)k, hipMemcpyDeviceToDevice, stream));
            if (paired) {
                WC_HIP(hipMemcpyAsync(mate_g + to, (const int32_t *)h->mate + from, 4 * (size_t)k, hipMemcpyDeviceToDevice, stream));
                WC_HIP(hipMemcpyAsync(flag_g + to, (const uint16_t *)h->flag + from, 2 * (size_t)k, hipMemcpyDeviceToDevice, stream));
            }
        }
        pos = ctx->tmp_a.as<int32_t>();
        mapq = ctx->tmp_b.as<uint8_t>();
        mate = mate_g;
        flag = flag_g;
    }
    rc = wc_convert_reads_ex_dev(ctx, stream, pos, mapq, paired ? flag : nullptr, paired ? mate : nullptr, ro.data(), n_chrom,
                                 binsize, min_shift, threshold, min_mapq, demand_pair, bin_offsets,
                                 reinterpret_cast<int32_t *>(stats_dev + 8), stats_dev);
    if (rc) return rc;
    return wc::convert_result(stream, stats_dev, bins, counts_out, stats_out, true);
}

}  // extern "C"
