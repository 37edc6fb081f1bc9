// Deflate and CRC-32 of many rows on the GPU, equally long or of lengths read on the device, in one of two framings
// (DESIGN.md 6c).  RAW: a row is one raw deflate stream (`testbatch -encoder gpu`, the page exports, `exportjson -gz`).
// BGZF: every block of a row is a deflate stream of its own inside a BGZF block (header with its size, CRC-32, ISIZE), and
// the end-of-file block stands behind the row's last (`exporttracks -gz`).
//
//   k_df_encode<BGZF, LEN>  one workgroup per (row, block of DF_B input bytes), the grid sized by the longest row (LEN: the
//                           rows' lengths are read on the device): run-length tokens, the block's own Huffman code
//                           (dynamic header) or a stored block, byte-aligned, into the block's slot of a scratch
//                           image; the block's CRC-32 share (RAW: moved to the row's end)
//   k_df_gather<BGZF>       the blocks' bytes to their place in the row (prefix sum of the block lengths) with what
//                           the framing puts around them; the row's length, and with RAW its CRC-32
//   k_df_assemble           the .npy members results_r / results_z of a batch from their framing (a template with
//                           gaps) and the float64 rows on the device
//
// The strategy is zlib's Z_RLE at level 1: a run of equal bytes is one literal and distance-1 matches, nothing else is
// searched.  Every position decides its own token from the run it lies in, so a block is coded by 256 lanes at once;
// the two serial pieces (the Huffman construction on 286 and 19 symbols, huffman.h, and the header) run in one lane.
// Blocks end on a byte boundary (an empty stored block behind a coded one, as a zlib sync flush writes it), which is
// what lets them be coded independently and gathered afterwards.
#include <limits.h>

#include "ctx.h"
#include "huffman.h"

namespace {

const int DF_B = 16384;             // input bytes per block
const int DF_T = 256;               // lanes per workgroup; each owns DF_B / DF_T = 64 consecutive bytes
const int DF_SLICE = DF_B / DF_T;
const int DF_PITCH = DF_SLICE + 4;  // LDS bytes per slice: 17 words, so the lanes' slices start in different banks
const int DF_CAP = DF_B + 16;       // bytes of a block's slot in the scratch image (a block takes at most DF_B + 5)
const int DF_MAX_GAPS = 64;

static_assert(DF_SLICE == 64, "a lane's heads are one 64-bit mask");

// a * b modulo the CRC-32 polynomial, reflected bit order (bit 31 is x^0): zlib's multmodp
__host__ __device__ constexpr uint32_t df_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b >> 1) ^ ((b & 1u) ? 0xEDB88320u : 0u);
    }
    return p;
}
struct DfPow {
    uint32_t v[48];                 // x^(8 * 2^k) modulo the polynomial
    constexpr DfPow() : v{} {
        uint32_t p = 0x00800000u;   // x^8
        for (int k = 0; k < 48; ++k) { v[k] = p; p = df_mulmod(p, p); }
    }
};
__constant__ DfPow df_pow = DfPow();
__constant__ uint8_t df_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// x^(8 m): what m further bytes multiply a CRC register by
__device__ inline uint32_t df_xpow8(uint64_t m) {
    uint32_t p = 0x80000000u;       // x^0
#pragma unroll 1
    for (int k = 0; m; ++k, m >>= 1)
        if (m & 1u) p = df_mulmod(df_pow.v[k], p);
    return p;
}

struct DfLds {
    uint8_t data[DF_T * DF_PITCH];  // the block's input, slice by slice
    uint32_t out[DF_CAP / 4];       // the coded block, bit by bit
    uint32_t crc_tab[256];
    uint32_t lfreq[wc::HUFF_MAX_SYMS];
    uint32_t lcode[wc::HUFF_MAX_SYMS];      // bit-reversed code | length << 16
    uint32_t cfreq[19], ccode[19];
    uint8_t llen[wc::HUFF_MAX_SYMS];
    uint8_t clen[20];
    uint8_t cl_sym[320], cl_extra[320];     // the code lengths, run-length coded with 16 / 17 / 18
    int wtot[4];
    int n_cl, header_bits, body_bits;
    uint32_t crc;
    wc::HuffWork hw;
};

// Exclusive scan over the workgroup's 256 lanes (REV: over the lanes above, instead of the lanes below).
template <bool REV, class Op> __device__ __forceinline__ int df_scan(int v, int ident, int *wtot, Op op, int t) {
    const int lane = t & 63, wv = t >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int x = REV ? __shfl_down(inc, d) : __shfl_up(inc, d);
        if (REV ? lane + d < 64 : lane >= d) inc = op(inc, x);
    }
    if (lane == (REV ? 0 : 63)) wtot[wv] = inc;
    wc_sync();
    int base = ident;
    for (int k = 0; k < 4; ++k)
        if (REV ? k > wv : k < wv) base = op(base, wtot[k]);
    int ex = REV ? __shfl_down(inc, 1) : __shfl_up(inc, 1);
    if (lane == (REV ? 63 : 0)) ex = ident;
    wc_sync();                      // wtot is free for the next scan
    return op(base, ex);
}

struct DfBits {                     // a lane's own stretch of the bit stream: whole words leave through atomic OR
    uint32_t *out;
    uint64_t acc;
    int nb, wi;
    __device__ __forceinline__ void start(uint32_t *o, int bitpos) { out = o; wi = bitpos >> 5; nb = bitpos & 31; acc = 0; }
    __device__ __forceinline__ void put(uint32_t v, int n) {
        acc |= (uint64_t)v << nb;
        nb += n;
        if (nb >= 32) {
            atomicOr(&out[wi++], (uint32_t)acc);
            acc >>= 32;
            nb -= 32;
        }
    }
    __device__ __forceinline__ void flush() {
        if (nb) atomicOr(&out[wi], (uint32_t)acc);
        nb = 0;
        acc = 0;
    }
};

// length symbol of a match of `len` bytes (3 .. 258), its extra bits and their number
__device__ __forceinline__ int df_len_sym(int len, int &extra, int &nextra) {
    const int L = len - 3;
    extra = 0;
    nextra = 0;
    if (L < 8) return 257 + L;
    if (L == 255) return 285;
    nextra = 29 - __clz(L);         // 8 .. 15: 1 bit, 16 .. 31: 2 bits, ... 128 .. 254: 5 bits
    extra = L & ((1 << nextra) - 1);
    return 261 + 4 * nextra + ((L >> nextra) & 3);
}

// The tokens of one lane's 64 positions, in order: f(symbol, extra, nextra, is_match).  hm: the positions of the slice at
// which a run starts (a byte that differs from the one before it, the block's first byte, and everything from n on);
// run_start / run_end: the last run start below the slice and the first one above it.  A run of L equal bytes is a
// literal and L - 1 bytes of distance-1 matches, cut into pieces of 258; a last piece of 1 or 2 bytes is literals.
template <class F> __device__ __forceinline__ void df_tokens(const uint8_t *slice, uint64_t hm, int run_start, int run_end,
                                                             int p0, int n, F f) {
#pragma unroll 1
    for (int k = 0; k < DF_SLICE; ++k) {
        const int i = p0 + k;
        if (i >= n) break;
        const uint64_t below = hm & (~0ull >> (63 - k));
        const int s = below ? p0 + 63 - __clzll((long long)below) : run_start;
        const uint64_t above = k < 63 ? hm >> (k + 1) : 0ull;
        const int e = above ? i + 1 + (__ffsll((unsigned long long)above) - 1) : run_end;
        const int off = i - s;
        bool literal = off == 0;
        if (!literal) {
            const int j = off - 1, rest = e - s - 1;
            const int q = j / 258;
            const int left = rest - q * 258, piece = left < 258 ? left : 258;
            if (piece < 3) literal = true;
            else if (j == q * 258) {
                int extra, nextra;
                const int sym = df_len_sym(piece, extra, nextra);
                f(sym, extra, nextra, true);
            }
        }
        if (literal) f((int)slice[k], 0, 0, false);
    }
}

// One block: the n bytes at `in` coded into `slot`, its length into *len_out, and into *crc_out the block's CRC-32 share
// (register started at zero) moved `behind` bytes on: to the end of the stream the block is part of, 0 for the block's own.
// final_blk: the deflate stream ends with this block.
__device__ __forceinline__ void df_encode_block(DfLds &S, const uint8_t *__restrict__ in, const int n, const bool final_blk,
                                                const long long behind, uint8_t *__restrict__ slot, int *__restrict__ len_out,
                                                uint32_t *__restrict__ crc_out) {
    const int t = threadIdx.x;
    {
        uint32_t c = (uint32_t)t;
        for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
        S.crc_tab[t] = c;
    }
    for (int i = t; i < wc::HUFF_MAX_SYMS; i += DF_T) S.lfreq[i] = 0;
    for (int i = t; i < DF_CAP / 4; i += DF_T) S.out[i] = 0;
    if (t < 19) S.cfreq[t] = 0;
    if ((reinterpret_cast<uintptr_t>(in) & 3u) == 0) {
        const uint32_t *in32 = reinterpret_cast<const uint32_t *>(in);
        for (int w = t; w < (n >> 2); w += DF_T) {
            const int i = 4 * w;
            *reinterpret_cast<uint32_t *>(&S.data[(i >> 6) * DF_PITCH + (i & 63)]) = in32[w];
        }
        for (int i = (n & ~3) + t; i < n; i += DF_T) S.data[(i >> 6) * DF_PITCH + (i & 63)] = in[i];
    } else {
        for (int i = t; i < n; i += DF_T) S.data[(i >> 6) * DF_PITCH + (i & 63)] = in[i];
    }
    wc_sync();

    // ---- run starts of this lane's slice, and the slice's share of the CRC ----
    const int p0 = t * DF_SLICE;
    const uint8_t *slice = &S.data[t * DF_PITCH];
    uint64_t hm = 0;
    uint32_t c = 0;
    {
        uint32_t prev = t > 0 ? S.data[(t - 1) * DF_PITCH + 63] : 0u;
#pragma unroll 4
        for (int j = 0; j < DF_SLICE / 4; ++j) {
            uint32_t word = reinterpret_cast<const uint32_t *>(slice)[j];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * j + q, i = p0 + k;
                const uint32_t cur = word & 0xFFu;
                word >>= 8;
                if (i >= n || i == 0 || cur != prev) hm |= 1ull << k;
                if (i < n) c = S.crc_tab[(c ^ cur) & 0xFFu] ^ (c >> 8);
                prev = cur;
            }
        }
    }
    {
        // crc(A B) = crc(A) x^(8 |B|) + crc(B) for registers that start at zero: the slice's bytes, moved to the block's end
        const int end = p0 + DF_SLICE < n ? p0 + DF_SLICE : n;
        if (c) c = df_mulmod(df_xpow8((uint64_t)(n - end)), c);
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) c ^= (uint32_t)__shfl_xor((int)c, d);
        if ((t & 63) == 0) S.wtot[t >> 6] = (int)c;
        wc_sync();
        if (t == 0) {
            const uint32_t x = (uint32_t)(S.wtot[0] ^ S.wtot[1] ^ S.wtot[2] ^ S.wtot[3]);
            S.crc = x ? df_mulmod(df_xpow8((uint64_t)behind), x) : 0u;       // ... and to the stream's end
        }
        wc_sync();
    }
    const int last_head = hm ? p0 + 63 - __clzll((long long)hm) : -1;
    const int first_head = hm ? p0 + (__ffsll((unsigned long long)hm) - 1) : DF_B;
    const int run_start = df_scan<false>(last_head, -1, S.wtot, [](int a, int x) { return a > x ? a : x; }, t);
    const int run_end = df_scan<true>(first_head, DF_B, S.wtot, [](int a, int x) { return a < x ? a : x; }, t);

    // ---- histogram, code lengths, header (lane 0), codes ----
    df_tokens(slice, hm, run_start, run_end, p0, n, [&](int sym, int, int, bool) { atomicAdd(&S.lfreq[sym], 1u); });
    wc_sync();
    if (t == 0) {
        S.lfreq[256] = 1;
        wc::huffman_lengths(S.lfreq, 286, 15, S.llen, S.hw);
        int hlit = 286;
        while (hlit > 257 && S.llen[hlit - 1] == 0) --hlit;
        // the code lengths of the hlit literal/length symbols and of two distance symbols (1 bit each: only distance 1
        // occurs, and two codes make the set complete whether or not the block has a match), run-length coded
        const int total = hlit + 2;
        int n_cl = 0;
#pragma unroll 1
        for (int i = 0; i < total;) {
            const int v = i < hlit ? S.llen[i] : 1;
            int run = 1;
            while (i + run < total && (i + run < hlit ? S.llen[i + run] : 1) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) {
                    const int take = run < 138 ? run : 138;
                    S.cl_sym[n_cl] = 18; S.cl_extra[n_cl++] = (uint8_t)(take - 11);
                    run -= take;
                }
                if (run >= 3) { S.cl_sym[n_cl] = 17; S.cl_extra[n_cl++] = (uint8_t)(run - 3); run = 0; }
            } else {
                S.cl_sym[n_cl] = (uint8_t)v; S.cl_extra[n_cl++] = 0;
                --run;
                while (run >= 3) {
                    const int take = run < 6 ? run : 6;
                    S.cl_sym[n_cl] = 16; S.cl_extra[n_cl++] = (uint8_t)(take - 3);
                    run -= take;
                }
            }
            for (; run > 0; --run) { S.cl_sym[n_cl] = (uint8_t)v; S.cl_extra[n_cl++] = 0; }
        }
        for (int i = 0; i < n_cl; ++i) S.cfreq[S.cl_sym[i]]++;
        wc::huffman_lengths(S.cfreq, 19, 7, S.clen, S.hw);
        int hclen = 19;
        while (hclen > 4 && S.clen[df_cl_order[hclen - 1]] == 0) --hclen;
        uint32_t code = 0;
        for (int l = 1; l <= 7; ++l) {
            for (int s = 0; s < 19; ++s)
                if (S.clen[s] == l) S.ccode[s] = __brev(code++) >> (32 - l);
            code <<= 1;
        }
        DfBits w;
        w.start(S.out, 0);
        w.put(final_blk ? 1u : 0u, 1);
        w.put(2u, 2);
        w.put((uint32_t)(hlit - 257), 5);
        w.put(1u, 5);
        w.put((uint32_t)(hclen - 4), 4);
        int bits = 17 + 3 * hclen;
        for (int i = 0; i < hclen; ++i) w.put(S.clen[df_cl_order[i]], 3);
#pragma unroll 1
        for (int i = 0; i < n_cl; ++i) {
            const int s = S.cl_sym[i];
            w.put(S.ccode[s], S.clen[s]);
            bits += S.clen[s];
            if (s >= 16) {
                const int ne = s == 16 ? 2 : s == 17 ? 3 : 7;
                w.put(S.cl_extra[i], ne);
                bits += ne;
            }
        }
        w.flush();
        S.header_bits = bits;
    }
    wc_sync();
    for (int sym = t; sym < 286; sym += DF_T) {
        const int l = S.llen[sym];
        uint32_t code = 0;
        for (int o = 0; o < 286; ++o) {
            const int lo = S.llen[o];
            if (lo && lo < l) code += 1u << (l - lo);
            else if (lo == l && o < sym) ++code;
        }
        S.lcode[sym] = l ? (__brev(code) >> (32 - l)) | ((uint32_t)l << 16) : 0u;
    }
    wc_sync();

    // ---- where every lane's bits go; coded or stored ----
    int my_bits = 0;
    df_tokens(slice, hm, run_start, run_end, p0, n, [&](int sym, int, int nextra, bool match) {
        my_bits += (int)(S.lcode[sym] >> 16) + (match ? nextra + 1 : 0);
    });
    const int before = df_scan<false>(my_bits, 0, S.wtot, [](int a, int x) { return a + x; }, t);
    if (t == DF_T - 1) S.body_bits = before + my_bits;
    wc_sync();
    const int eob_at = S.header_bits + S.body_bits;
    const int total_bits = eob_at + (int)(S.lcode[256] >> 16);
    // behind a coded block that is not the last: the header of an empty stored block (three zero bits), the padding to
    // a whole byte, and its length words 00 00 FF FF
    const int marker_at = (total_bits + 3 + 7) >> 3;
    const int coded_bytes = final_blk ? (total_bits + 7) >> 3 : marker_at + 4;
    const int stored_bytes = 5 + n;
    const bool coded = n > 0 && coded_bytes < stored_bytes;
    if (coded) {
        DfBits w;
        w.start(S.out, S.header_bits + before);
        df_tokens(slice, hm, run_start, run_end, p0, n, [&](int sym, int extra, int nextra, bool match) {
            const uint32_t e = S.lcode[sym];
            w.put(e & 0xFFFFu, (int)(e >> 16));
            if (match) w.put((uint32_t)extra, nextra + 1);      // the extra bits, then distance symbol 0: one zero bit
        });
        if (t == DF_T - 1) {
            const uint32_t e = S.lcode[256];
            w.put(e & 0xFFFFu, (int)(e >> 16));
            if (!final_blk) {
                w.flush();
                w.start(S.out, (marker_at + 2) * 8);
                w.put(0xFFFFu, 16);
            }
        }
        w.flush();
        wc_sync();
        for (int i = t; i < (coded_bytes + 3) >> 2; i += DF_T) reinterpret_cast<uint32_t *>(slot)[i] = S.out[i];
    } else {
        const uint32_t len = (uint32_t)n;
        for (int i = t; i < stored_bytes; i += DF_T) {
            uint8_t v;
            if (i >= 5) v = S.data[((i - 5) >> 6) * DF_PITCH + ((i - 5) & 63)];
            else v = i == 0 ? (final_blk ? 1 : 0) : i == 1 ? (len & 0xFFu) : i == 2 ? (len >> 8) : i == 3 ? (~len & 0xFFu) : ((~len >> 8) & 0xFFu);
            slot[i] = v;
        }
    }
    if (t == 0) {
        *len_out = coded ? coded_bytes : stored_bytes;
        *crc_out = S.crc;
    }
}

// BGZF (the SAM specification, section 4.1): every block of a row is a gzip member of its own with the extra field BC
// that holds the member's size, and the 28-byte empty member ends the file.
const int BZ_HEAD = 18, BZ_TAIL = 8, BZ_EOF = 28;
__constant__ uint8_t bz_eof[BZ_EOF] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};

// blocks of a row of `len` bytes: an empty row is one empty final block of a raw stream and no BGZF block at all; -1 for
// a length outside 0 .. max_row_bytes
template <bool BGZF> __device__ __forceinline__ long long df_blocks(long long len, long long max_row_bytes) {
    if (len < 0 || len > max_row_bytes) return -1;
    return !BGZF && len == 0 ? 1 : (len + DF_B - 1) / DF_B;
}

// Workgroup (row, b) of a grid of n_blk blocks per row, enough for max_row_bytes: block b of the row's bytes.  LEN: the
// row has row_len[row] bytes and blocks behind its end do nothing; otherwise every row has max_row_bytes and fills the
// grid.  RAW: the deflate stream ends with the row's last block, and the CRC-32 shares are moved to the row's end.
// BGZF: every block is a stream of its own.  (LEN is a template parameter because the fixed-length kernel, 50 KB of
// code, ran 1 % slower with the length's source chosen at run time: EXPERIMENTS.md.)
template <bool BGZF, bool LEN>
__global__ void __launch_bounds__(DF_T) k_df_encode(const uint8_t *__restrict__ src, const long long *__restrict__ row_len,
                                                    long long max_row_bytes, long long src_stride, int n_blk,
                                                    uint8_t *__restrict__ scratch, int *__restrict__ blk_len,
                                                    uint32_t *__restrict__ blk_crc) {
    __shared__ DfLds S;
    const long long id = blockIdx.x;
    const long long row = id / n_blk;
    const int b = (int)(id - row * n_blk);
    const long long len = LEN ? row_len[row] : max_row_bytes;
    const int nb = LEN ? (int)df_blocks<BGZF>(len, max_row_bytes) : n_blk;  // (at most n_blk)
    if (LEN && b >= nb) return;                                // (the same in every lane)
    const long long start = (long long)b * DF_B;
    const int n = (int)(len - start < DF_B ? len - start : DF_B);                   // 0 only in an empty row
    df_encode_block(S, src + row * src_stride + start, n, BGZF || b == nb - 1, BGZF ? 0 : len - start - n, scratch + id * DF_CAP,
                    &blk_len[id], &blk_crc[id]);
}

// len bytes of a scratch slot to `to`.  The destination is arbitrary to the byte, the slot is 16-byte aligned: whole
// destination words are put together from two source words.
__device__ __forceinline__ void df_copy_block(const uint8_t *__restrict__ from, uint8_t *__restrict__ to, const int len, const int t) {
    int head = (int)((4u - (unsigned)(reinterpret_cast<uintptr_t>(to) & 3u)) & 3u);
    if (head > len) head = len;
    const int words = (len - head) >> 2;
    if (t < head) to[t] = from[t];
    const uint32_t *from32 = reinterpret_cast<const uint32_t *>(from);
    uint32_t *to32 = reinterpret_cast<uint32_t *>(to + head);
    const int sh = 8 * (head & 3);
    for (int w = t; w < words; w += DF_T) {
        const int at = (head >> 2) + w;         // (head < 4: at == w; the second word stays inside the slot, DF_CAP - DF_B - 5 > 7)
        const uint32_t lo = from32[at], hi = from32[at + 1];
        to32[w] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
    }
    const int done = head + 4 * words;
    if (t < len - done) to[done + t] = from[done + t];
}

// Block (row, b): its bytes from the scratch slot to their place in the row at out + row * out_stride, the sum of what the
// row's blocks before it take.  RAW: the streams alone, and the row's last block leaves the row's length and CRC-32.
// BGZF: BZ_HEAD + the stream + BZ_TAIL per block, and the row's last block (block 0 of an empty row, which has none) also
// leaves the end-of-file block and the row's length.  out_len[row] = -1 and nothing else for a length out of range.
template <bool BGZF>
__global__ void __launch_bounds__(DF_T) k_df_gather(const uint8_t *__restrict__ scratch, const int *__restrict__ blk_len,
                                                    const uint32_t *__restrict__ blk_crc, const long long *__restrict__ row_len,
                                                    long long max_row_bytes, int n_blk, uint8_t *__restrict__ out, long long out_stride,
                                                    long long *__restrict__ out_len, uint32_t *__restrict__ crc_out) {
    __shared__ long long s_off[4];
    __shared__ uint32_t s_crc[4];
    const int t = threadIdx.x;
    const long long id = blockIdx.x;
    const long long row = id / n_blk;
    const int b = (int)(id - row * n_blk);
    const long long rlen = row_len ? row_len[row] : max_row_bytes;
    const long long nb = df_blocks<BGZF>(rlen, max_row_bytes);
    uint8_t *base = out + row * out_stride;
    if (nb <= 0) {
        if (b == 0 && nb == 0 && t < BZ_EOF) base[t] = bz_eof[t];
        if (b == 0 && t == 0) out_len[row] = nb == 0 ? BZ_EOF : -1;
        return;
    }
    if (b >= nb) return;
    const int around = BGZF ? BZ_HEAD + BZ_TAIL : 0;
    long long off = 0;
    uint32_t x = 0;
    for (int k = t; k <= b; k += DF_T) {
        if (k < b) off += blk_len[row * n_blk + k] + around;
        if (!BGZF) x ^= blk_crc[row * n_blk + k];
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        off += __shfl_xor(off, d);
        if (!BGZF) x ^= (uint32_t)__shfl_xor((int)x, d);
    }
    if ((t & 63) == 0) {
        s_off[t >> 6] = off;
        if (!BGZF) s_crc[t >> 6] = x;
    }
    wc_sync();
    off = s_off[0] + s_off[1] + s_off[2] + s_off[3];
    const int len = blk_len[id];
    const bool last = b == nb - 1;
    uint8_t *to = base + off;
    // the CRC registers started at zero; zlib's starts at all ones and is inverted at the end
    if (BGZF) {
        const long long start = (long long)b * DF_B;
        const uint32_t n = (uint32_t)(rlen - start < DF_B ? rlen - start : DF_B);
        if (t < BZ_HEAD) {
            const uint32_t bsize = (uint32_t)(BZ_HEAD + len + BZ_TAIL - 1);
            to[t] = t < 16 ? bz_eof[t] : (uint8_t)(bsize >> (8 * (t - 16)));
        } else if (t < BZ_HEAD + BZ_TAIL) {
            const uint32_t crc = blk_crc[id] ^ df_mulmod(df_xpow8((uint64_t)n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
            const int k = t - BZ_HEAD;
            to[BZ_HEAD + len + k] = (uint8_t)((k < 4 ? crc : n) >> (8 * (k & 3)));
        } else if (last && t >= 64 && t < 64 + BZ_EOF) {
            to[BZ_HEAD + len + BZ_TAIL + (t - 64)] = bz_eof[t - 64];
        }
        to += BZ_HEAD;
    } else if (last && t == 0) {
        x = s_crc[0] ^ s_crc[1] ^ s_crc[2] ^ s_crc[3];
        crc_out[row] = x ^ df_mulmod(df_xpow8((uint64_t)rlen), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
    }
    if (last && t == 0) out_len[row] = off + len + (BGZF ? around + BZ_EOF : 0);
    df_copy_block(scratch + id * DF_CAP, to, len, t);
}

// image[row, p] = the member's byte p: the template's, or inside gap c byte p - dst[c] of the doubles
// rows[row * row_stride + first[c] ...].  table: DEVICE int64 [3, n_gaps] = dst byte offsets, first elements, elements.
__global__ void __launch_bounds__(256) k_df_assemble(const uint8_t *__restrict__ tmpl, long long member_bytes,
                                                     const long long *__restrict__ table, int n_gaps, const double *__restrict__ rows,
                                                     long long row_stride, uint8_t *__restrict__ image, long long image_stride) {
    __shared__ long long s_dst[DF_MAX_GAPS], s_first[DF_MAX_GAPS], s_bytes[DF_MAX_GAPS];
    const int t = threadIdx.x;
    if (t < n_gaps) {
        s_dst[t] = table[t];
        s_first[t] = table[n_gaps + t];
        s_bytes[t] = 8 * table[2 * n_gaps + t];
    }
    wc_sync();
    const long long row = blockIdx.y;
    const long long w = (long long)blockIdx.x * 256 + t;
    if (4 * w >= image_stride) return;
    const uint8_t *values = reinterpret_cast<const uint8_t *>(rows + row * row_stride);
    uint32_t word = 0;
    for (int q = 0; q < 4; ++q) {
        const long long p = 4 * w + q;
        uint32_t v = 0;
        if (p < member_bytes) {
            v = tmpl[p];
            for (int g = 0; g < n_gaps; ++g) {
                const long long rel = p - s_dst[g];
                if (rel >= 0 && rel < s_bytes[g]) v = values[8 * s_first[g] + rel];
            }
        }
        word |= v << (8 * q);
    }
    reinterpret_cast<uint32_t *>(image + row * image_stride)[w] = word;
}

// ---- the host's half: one check, one enqueue and one staging wrapper for both framings --------------------------------
struct DfFrame {
    bool bgzf;
    const char *name, *bound_name;      // the words of the messages
    int64_t (*bound)(int64_t);
    int64_t least;                      // bytes of the shortest row there is: a final block, the end-of-file block
};
const DfFrame DF_RAW = {false, "deflate", "wc_deflate_bound", wc_deflate_bound, 1};
const DfFrame DF_BGZF = {true, "bgzf", "wc_bgzf_bound", wc_bgzf_bound, BZ_EOF};

// row_len (may be NULL: every row has row_bytes bytes) is not looked into: it may be a device array
int df_check(const wc_ctx *ctx, const DfFrame &f, const unsigned char *src, int64_t n_rows, const int64_t *row_len, int64_t row_bytes,
             int64_t src_stride, const unsigned char *out, int64_t out_stride, const int64_t *out_len, const uint32_t *crc) {
    WC_CHECK(ctx && n_rows >= 0 && row_bytes >= 0 && src_stride >= row_bytes && (src || n_rows == 0 || row_bytes == 0) &&
                 (n_rows == 0 || (out && out_len && (f.bgzf ? row_len != nullptr : crc != nullptr))),
             WC_E_ARG, "%s: unusable argument", f.name);
    WC_CHECK(out_stride >= f.bound(row_bytes), WC_E_ARG, "%s: %lld bytes per output row, %s(%lld) is %lld", f.name, (long long)out_stride,
             f.bound_name, (long long)row_bytes, (long long)f.bound(row_bytes));
    return WC_OK;
}

// the two kernels, enqueued (DEVICE pointers): rows of row_len[i] <= row_bytes bytes, or without row_len of row_bytes
int df_enqueue(wc_ctx *ctx, hipStream_t stream, const DfFrame &f, const unsigned char *src, int64_t n_rows, const int64_t *row_len,
               int64_t row_bytes, int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len, uint32_t *crc) {
    int rc;
    if ((rc = df_check(ctx, f, src, n_rows, row_len, row_bytes, src_stride, out, out_stride, out_len, crc))) return rc;
    if (n_rows == 0) return WC_OK;
    const int64_t n_blk = row_bytes <= 0 ? 1 : (row_bytes + DF_B - 1) / DF_B;
    WC_CHECK(n_blk <= INT_MAX / 2 && n_rows <= (int64_t)INT_MAX / n_blk, WC_E_LIMIT, "%s: %lld rows of %s%lld blocks in one call", f.name,
             (long long)n_rows, row_len ? "up to " : "", (long long)n_blk);
    const int64_t total = n_rows * n_blk;
    WC_HIP(hipSetDevice(ctx->device));
    if ((rc = ctx->df_scratch.reserve((size_t)total * DF_CAP)) || (rc = ctx->df_meta.reserve((size_t)total * 8))) return rc;
    int *blk_len = ctx->df_meta.as<int>();
    uint32_t *blk_crc = ctx->df_meta.as<uint32_t>() + total;
    const auto encode = !row_len ? k_df_encode<false, false> : f.bgzf ? k_df_encode<true, true> : k_df_encode<false, true>;
    hipLaunchKernelGGL(encode, dim3((unsigned)total), dim3(DF_T), 0, stream, (const uint8_t *)src, (const long long *)row_len,
                       (long long)row_bytes, (long long)src_stride, (int)n_blk, ctx->df_scratch.as<uint8_t>(), blk_len, blk_crc);
    WC_HIP(hipGetLastError());
    hipLaunchKernelGGL(f.bgzf ? k_df_gather<true> : k_df_gather<false>, dim3((unsigned)total), dim3(DF_T), 0, stream,
                       (const uint8_t *)ctx->df_scratch.as<uint8_t>(), (const int *)blk_len, (const uint32_t *)blk_crc,
                       (const long long *)row_len, (long long)row_bytes, (int)n_blk, (uint8_t *)out, (long long)out_stride,
                       (long long *)out_len, crc);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

// the same from HOST pointers, synchronising; crc may be NULL where the framing has none
int df_stage(wc_ctx *ctx, const DfFrame &f, const unsigned char *src, int64_t n_rows, const int64_t *row_len, int64_t row_bytes,
             int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len, uint32_t *crc) {
    int rc;
    if ((rc = df_check(ctx, f, src, n_rows, row_len, row_bytes, src_stride, out, out_stride, out_len, crc))) return rc;
    for (int64_t i = 0; row_len && i < n_rows; ++i)
        WC_CHECK(row_len[i] >= 0 && row_len[i] <= row_bytes, WC_E_ARG, "%s: row %lld has %lld bytes, max_row_bytes is %lld", f.name,
                 (long long)i, (long long)row_len[i], (long long)row_bytes);
    if (n_rows == 0) return WC_OK;
    WC_HIP(hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)((n_rows - 1) * src_stride + (row_len ? row_len[n_rows - 1] : row_bytes));
    if ((rc = ctx->tmp_a.reserve(in_bytes + 4)) || (rc = ctx->tmp_b.reserve((size_t)(n_rows * out_stride))) ||
        (rc = ctx->tmp_c.reserve((size_t)n_rows * 8)) || (rc = ctx->tmp_d.reserve((size_t)n_rows * 12)))
        return rc;
    int64_t *d_len = ctx->tmp_d.as<int64_t>();
    uint32_t *d_crc = reinterpret_cast<uint32_t *>(d_len + n_rows);
    if (in_bytes) WC_HIP(hipMemcpy(ctx->tmp_a.p, src, in_bytes, hipMemcpyHostToDevice));
    if (row_len) WC_HIP(hipMemcpy(d_len, row_len, (size_t)n_rows * 8, hipMemcpyHostToDevice));
    if ((rc = df_enqueue(ctx, nullptr, f, ctx->tmp_a.as<unsigned char>(), n_rows, row_len ? d_len : nullptr, row_bytes, src_stride,
                         ctx->tmp_b.as<unsigned char>(), out_stride, ctx->tmp_c.as<int64_t>(), d_crc)))
        return rc;
    WC_HIP(hipMemcpy(out_len, ctx->tmp_c.p, (size_t)n_rows * 8, hipMemcpyDeviceToHost));
    if (crc) WC_HIP(hipMemcpy(crc, d_crc, (size_t)n_rows * 4, hipMemcpyDeviceToHost));
    // only the rows' own bytes: what lies behind them is whatever the staging buffer held
    for (int64_t i = 0; i < n_rows; ++i) {
        WC_CHECK(out_len[i] >= f.least && out_len[i] <= out_stride, WC_E_INTERNAL, "%s: a row of %lld bytes", f.name, (long long)out_len[i]);
        WC_HIP(hipMemcpy(out + i * out_stride, ctx->tmp_b.as<unsigned char>() + i * out_stride, (size_t)out_len[i], hipMemcpyDeviceToHost));
    }
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_deflate_block_bytes(void) { return DF_B; }

int64_t wc_deflate_bound(int64_t row_bytes) {
    if (row_bytes < 0) return -1;
    return row_bytes + 10 * ((row_bytes + DF_B - 1) / DF_B + 1);
}

int wc_huffman_lengths(const uint32_t *freq, int n, int limit, uint8_t *len_out) {
    WC_CHECK(freq && len_out && n >= 0 && n <= wc::HUFF_MAX_SYMS && limit >= 1 && limit <= 15, WC_E_ARG,
             "huffman: %d symbols (at most %d), limit %d (1 .. 15)", n, wc::HUFF_MAX_SYMS, limit);
    int used = 0;
    for (int s = 0; s < n; ++s) used += freq[s] != 0;
    WC_CHECK(used <= (1 << limit), WC_E_ARG, "huffman: %d used symbols have no code of at most %d bits", used, limit);
    wc::HuffWork work;
    wc::huffman_lengths(freq, n, limit, len_out, work);
    return WC_OK;
}

int wc_deflate_rows_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, int64_t row_bytes, int64_t src_stride,
                        unsigned char *out, int64_t out_stride, int64_t *out_len, uint32_t *crc) {
    return df_enqueue(ctx, (hipStream_t)stream, DF_RAW, src, n_rows, nullptr, row_bytes, src_stride, out, out_stride, out_len, crc);
}

int wc_deflate_rows_len_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, const int64_t *row_len,
                            int64_t max_row_bytes, int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len,
                            uint32_t *crc) {
    WC_CHECK(row_len || n_rows <= 0, WC_E_ARG, "deflate: unusable argument");
    return df_enqueue(ctx, (hipStream_t)stream, DF_RAW, src, n_rows, row_len, max_row_bytes, src_stride, out, out_stride, out_len, crc);
}

int wc_deflate_rows(wc_ctx *ctx, const unsigned char *src, int64_t n_rows, int64_t row_bytes, int64_t src_stride, unsigned char *out,
                    int64_t out_stride, int64_t *out_len, uint32_t *crc) {
    return df_stage(ctx, DF_RAW, src, n_rows, nullptr, row_bytes, src_stride, out, out_stride, out_len, crc);
}

int64_t wc_bgzf_bound(int64_t row_bytes) {
    if (row_bytes < 0) return -1;
    return row_bytes + (BZ_HEAD + 5 + BZ_TAIL) * ((row_bytes + DF_B - 1) / DF_B) + BZ_EOF;
}

int wc_bgzf_rows_dev(wc_ctx *ctx, void *stream, const unsigned char *src, int64_t n_rows, const int64_t *row_len, int64_t max_row_bytes,
                     int64_t src_stride, unsigned char *out, int64_t out_stride, int64_t *out_len) {
    return df_enqueue(ctx, (hipStream_t)stream, DF_BGZF, src, n_rows, row_len, max_row_bytes, src_stride, out, out_stride, out_len, nullptr);
}

int wc_bgzf_rows(wc_ctx *ctx, const unsigned char *src, int64_t n_rows, const int64_t *row_len, int64_t max_row_bytes, int64_t src_stride,
                 unsigned char *out, int64_t out_stride, int64_t *out_len) {
    return df_stage(ctx, DF_BGZF, src, n_rows, row_len, max_row_bytes, src_stride, out, out_stride, out_len, nullptr);
}

int wc_results_members_dev(wc_ctx *ctx, void *stream_, const unsigned char *tmpl, int64_t member_bytes, const int64_t *table,
                           int n_gaps, const double *rows, int64_t row_stride, int64_t n_rows, unsigned char *image,
                           int64_t image_stride) {
    WC_CHECK(ctx && tmpl && table && member_bytes > 0 && n_gaps >= 0 && n_gaps <= DF_MAX_GAPS && n_rows >= 0 && n_rows <= 65535 &&
                 (rows || n_gaps == 0) && image && image_stride >= member_bytes && image_stride % 4 == 0 &&
                 (reinterpret_cast<uintptr_t>(image) & 3u) == 0,
             WC_E_ARG, "members: unusable argument (at most %d gaps and 65535 rows; the image's rows start on 4-byte boundaries)",
             DF_MAX_GAPS);
    if (n_rows == 0) return WC_OK;
    WC_HIP(hipSetDevice(ctx->device));
    const int64_t words = image_stride / 4;
    hipLaunchKernelGGL(k_df_assemble, dim3((unsigned)((words + 255) / 256), (unsigned)n_rows), dim3(256), 0, (hipStream_t)stream_,
                       (const uint8_t *)tmpl, (long long)member_bytes, (const long long *)table, n_gaps, rows, (long long)row_stride,
                       (uint8_t *)image, (long long)image_stride);
    WC_HIP(hipGetLastError());
    return WC_OK;
}

}  // extern "C"
