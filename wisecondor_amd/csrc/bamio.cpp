// Native BAM reader for `convert` (the reference goes through pysam, wisetools.py:134-155): BGZF blocks inflated by a
// pool of threads, records walked by their block_size chain (records cross block boundaries), output as
// structure-of-arrays in file order = grouped by reference: pos[], mapq[], flag[], mate_pos[], per-reference offsets,
// names and lengths from the header.  No index file is needed.
//
// The three record counts of the `quality` dict come from the records themselves instead of pysam's index statistics:
//   mapped = refID >= 0 and flag 0x4 clear;  no_coordinate = refID < 0;  unmapped = flag 0x4 set
// (pysam documents its `unmapped` as including the reads without coordinates).  pysam is not available where this was
// written, so this one mapping is NOT verified against it.  The same holds for the paired-end fields: flag bits 0x2 /
// 0x40 stand for pysam's is_proper_pair / is_read1 and next_pos (record offset 24) for next_reference_start, after the
// SAM specification.
//
// The file is read in chunks of WC_BAM_CHUNK blocks: compressed bytes in, blocks inflated in parallel into one buffer,
// records parsed from it, the unfinished tail of the buffer carried to the front of the next chunk.  Errors, never
// crashes: every length is checked against the bytes that are there.  No GPU code in this file.
#include <zlib.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/wisecondor_hip.h"

namespace wc {
void set_error(const char *fmt, ...);
}

struct wc_bam {
    std::vector<std::string> names;
    std::vector<int64_t> lengths, offsets;      // offsets: n_refs + 1
    std::vector<int32_t> pos;
    std::vector<uint8_t> mapq;
    std::vector<uint16_t> flag;
    std::vector<int32_t> mate_pos;
    int64_t mapped = 0, unmapped = 0, no_coordinate = 0, name_bytes = 0;
};

namespace {

const int WC_BAM_CHUNK = 1024;      // BGZF blocks (at most 64 KiB of data each) inflated per round

inline uint16_t rd16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const unsigned char *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

struct Block {
    size_t in_off, in_len, out_off;
    uint32_t crc, isize;
};

template <class F> void run_pool(int n, int threads, F work) {
    if (threads < 1) threads = 1;
    if (threads > n) threads = n;
    std::atomic<int> next(0);
    auto loop = [&]() { for (int i = next.fetch_add(1); i < n; i = next.fetch_add(1)) work(i); };
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(loop);
    loop();
    for (std::thread &t : pool) t.join();
}

bool inflate_block(const unsigned char *in, const Block &b, unsigned char *out) {
    unsigned char dummy = 0;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<unsigned char *>(in + b.in_off);
    zs.avail_in = (uInt)b.in_len;
    zs.next_out = b.isize ? out + b.out_off : &dummy;
    zs.avail_out = b.isize ? b.isize : 1;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == b.isize;
    inflateEnd(&zs);
    if (!ok) return false;
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), out + b.out_off, b.isize) == b.crc || (b.isize == 0 && b.crc == 0);
}

// Header, then records, from a growing stream: feed() takes the bytes that are there and returns how many it used up
// (whole header / whole records only), or -1 with `rc` and the error text set.
struct Parser {
    wc_bam &b;
    bool header_done = false;
    int32_t cur_ref = -1, last_pos = 0;
    int64_t records = 0;
    int rc = WC_OK;
    explicit Parser(wc_bam &bam) : b(bam) {}

    long long fail(int code) { rc = code; return -1; }

    long long feed(const unsigned char *p, size_t n) {
        size_t at = 0;
        if (!header_done) {
            if (n >= 4 && memcmp(p, "BAM\1", 4) != 0) {
                wc::set_error("bam: bad magic (the inflated data does not start with BAM\\1)");
                return fail(WC_E_FORMAT);
            }
            if (n < 12) return 0;
            const int32_t l_text = (int32_t)rd32(p + 4);
            if (l_text < 0) { wc::set_error("bam: negative header text length"); return fail(WC_E_FORMAT); }
            at = 8 + (size_t)l_text;
            if (n < at + 4) return 0;
            const int32_t n_ref = (int32_t)rd32(p + at);
            at += 4;
            if (n_ref < 0) { wc::set_error("bam: negative reference count"); return fail(WC_E_FORMAT); }
            std::vector<std::string> names;
            std::vector<int64_t> lengths;
            for (int32_t r = 0; r < n_ref; ++r) {
                if (n < at + 4) return 0;
                const int32_t l_name = (int32_t)rd32(p + at);
                if (l_name < 1) { wc::set_error("bam: reference %d has a name of %d bytes", r, l_name); return fail(WC_E_FORMAT); }
                if (n < at + 4 + (size_t)l_name + 4) return 0;
                names.emplace_back(reinterpret_cast<const char *>(p + at + 4), strnlen(reinterpret_cast<const char *>(p + at + 4), (size_t)l_name));
                lengths.push_back((int64_t)(int32_t)rd32(p + at + 4 + l_name));
                at += 8 + (size_t)l_name;
            }
            b.names.swap(names);
            b.lengths.swap(lengths);
            b.offsets.assign((size_t)n_ref + 1, 0);
            header_done = true;
        }
        const int32_t n_ref = (int32_t)b.names.size();
        while (n - at >= 4) {
            const int32_t bs = (int32_t)rd32(p + at);
            if (bs < 32) {
                wc::set_error("bam: record %lld has block_size %d, below its 32 fixed bytes", (long long)records, bs);
                return fail(WC_E_FORMAT);
            }
            if (n - at - 4 < (size_t)bs) break;
            const unsigned char *r = p + at + 4;
            const int32_t ref = (int32_t)rd32(r), ps = (int32_t)rd32(r + 4), l_seq = (int32_t)rd32(r + 16);
            const unsigned flag = rd16(r + 14);
            const int64_t need = 32 + (int64_t)r[8] + 4 * (int64_t)rd16(r + 12) + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq;
            if (l_seq < 0 || need > (int64_t)bs) {
                wc::set_error("bam: the fields of record %lld overrun its block_size (%lld > %d)", (long long)records,
                              (long long)need, bs);
                return fail(WC_E_FORMAT);
            }
            if (ref >= n_ref) {
                wc::set_error("bam: record %lld names reference %d of %d", (long long)records, ref, n_ref);
                return fail(WC_E_FORMAT);
            }
            if (flag & 4u) ++b.unmapped;
            if (ref < 0) {
                ++b.no_coordinate;
            } else {
                if (!(flag & 4u)) ++b.mapped;
                if (ref < cur_ref) {
                    wc::set_error("bam: not coordinate-sorted: record %lld of reference %d follows reference %d (the records "
                                  "of a reference must be contiguous, references in header order)", (long long)records, ref, cur_ref);
                    return fail(WC_E_ARG);
                }
                if (ref == cur_ref && ps < last_pos) {
                    wc::set_error("bam: not coordinate-sorted: position %d follows %d in reference %d (record %lld)", ps,
                                  last_pos, ref, (long long)records);
                    return fail(WC_E_ARG);
                }
                if (b.pos.size() >= (size_t)INT32_MAX) {
                    wc::set_error("bam: more than 2^31 - 1 placed records");
                    return fail(WC_E_LIMIT);
                }
                cur_ref = ref;
                last_pos = ps;
                b.pos.push_back(ps);
                b.mapq.push_back(r[9]);
                b.flag.push_back((uint16_t)flag);
                b.mate_pos.push_back((int32_t)rd32(r + 24));
                ++b.offsets[(size_t)ref + 1];
            }
            ++records;
            at += 4 + (size_t)bs;
        }
        return (long long)at;
    }
};

int read_bam(const char *path, int n_threads, wc_bam &bam) {
    FILE *f = fopen(path, "rb");
    if (!f) { wc::set_error("bam: cannot open %s", path); return WC_E_IO; }
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    std::vector<unsigned char> comp, plain;
    std::vector<Block> blocks;
    Parser parser(bam);
    size_t left = 0;            // unparsed bytes at the front of `plain`
    long long block_no = 0;
    bool eof = false;
    while (!eof) {
        comp.clear();
        blocks.clear();
        size_t out_bytes = left;
        while ((int)blocks.size() < WC_BAM_CHUNK) {
            unsigned char h[12];
            const size_t got = fread(h, 1, 12, f);
            if (got == 0) { eof = true; break; }
            if (got < 12) { wc::set_error("bam: truncated BGZF block %lld (header cut short)", block_no); return WC_E_FORMAT; }
            if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) {
                wc::set_error(block_no ? "bam: damaged BGZF block %lld (no gzip header with an extra field)"
                                       : "bam: bad magic: not a BGZF file (block %lld)", block_no);
                return WC_E_FORMAT;
            }
            const size_t xlen = rd16(h + 10), base = comp.size();
            comp.resize(base + xlen);
            if (xlen && fread(comp.data() + base, 1, xlen, f) != xlen) {
                wc::set_error("bam: truncated BGZF block %lld (extra field cut short)", block_no);
                return WC_E_FORMAT;
            }
            long bsize = -1;
            for (size_t q = 0; q + 4 <= xlen;) {
                const size_t slen = rd16(comp.data() + base + q + 2);
                if (comp[base + q] == 'B' && comp[base + q + 1] == 'C' && slen == 2 && q + 6 <= xlen) bsize = rd16(comp.data() + base + q + 4);
                q += 4 + slen;
            }
            const long rest = bsize + 1 - 12 - (long)xlen;
            if (bsize < 0 || rest < 8) { wc::set_error("bam: damaged BGZF block %lld (no usable BC size field)", block_no); return WC_E_FORMAT; }
            comp.resize(base + (size_t)rest);
            if (fread(comp.data() + base, 1, (size_t)rest, f) != (size_t)rest) {
                wc::set_error("bam: truncated BGZF block %lld (%ld bytes announced)", block_no, rest);
                return WC_E_FORMAT;
            }
            Block b;
            b.in_off = base;
            b.in_len = (size_t)rest - 8;
            b.crc = rd32(comp.data() + base + rest - 8);
            b.isize = rd32(comp.data() + base + rest - 4);
            if (b.isize > 65536) { wc::set_error("bam: damaged BGZF block %lld (%u bytes of data announced)", block_no, b.isize); return WC_E_FORMAT; }
            b.out_off = out_bytes;
            out_bytes += b.isize;
            blocks.push_back(b);
            ++block_no;
        }
        plain.resize(out_bytes + 1);
        std::atomic<int> bad(-1);
        run_pool((int)blocks.size(), n_threads, [&](int i) {
            if (!inflate_block(comp.data(), blocks[i], plain.data())) {
                int none = -1;
                bad.compare_exchange_strong(none, i);
            }
        });
        if (bad.load() >= 0) {
            wc::set_error("bam: damaged BGZF block %lld (inflate or CRC failed)", block_no - (long long)blocks.size() + bad.load());
            return WC_E_FORMAT;
        }
        const long long used = parser.feed(plain.data(), out_bytes);
        if (used < 0) return parser.rc;
        left = out_bytes - (size_t)used;
        if (used && left) memmove(plain.data(), plain.data() + used, left);
    }
    if (!parser.header_done) { wc::set_error("bam: truncated: the data ends inside the BAM header"); return WC_E_FORMAT; }
    if (left) { wc::set_error("bam: truncated: the last record overruns the data (%zu bytes left over)", left); return WC_E_FORMAT; }
    for (size_t r = 0; r < bam.names.size(); ++r) bam.offsets[r + 1] += bam.offsets[r];
    bam.name_bytes = 0;
    for (const std::string &s : bam.names) bam.name_bytes += (int64_t)s.size() + 1;
    return WC_OK;
}

}  // namespace

extern "C" {

int wc_bam_open(const char *path, int n_threads, wc_bam **out) {
    if (!path || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    *out = nullptr;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 64) n_threads = 64;
    wc_bam *bam = nullptr;
    int rc;
    try {
        bam = new wc_bam();
        rc = read_bam(path, n_threads, *bam);
    } catch (const std::exception &e) {
        wc::set_error("bam: %s", e.what());
        rc = WC_E_LIMIT;
    }
    if (rc != WC_OK) { delete bam; return rc; }
    *out = bam;
    return WC_OK;
}

int wc_bam_info(const wc_bam *bam, int64_t out[8]) {
    if (!bam || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    out[0] = (int64_t)bam->names.size();
    out[1] = (int64_t)bam->pos.size();
    out[2] = bam->mapped;
    out[3] = bam->unmapped;
    out[4] = bam->no_coordinate;
    out[5] = bam->name_bytes;
    out[6] = out[7] = 0;
    return WC_OK;
}

int wc_bam_refs(const wc_bam *bam, char *names_out, int64_t names_cap, int64_t *lengths_out, int64_t *offsets_out) {
    if (!bam || !names_out || !lengths_out || !offsets_out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    if (names_cap < bam->name_bytes) { wc::set_error("bam: %lld bytes of names, room for %lld", (long long)bam->name_bytes, (long long)names_cap); return WC_E_ARG; }
    char *w = names_out;
    for (size_t r = 0; r < bam->names.size(); ++r) {
        memcpy(w, bam->names[r].data(), bam->names[r].size());
        w += bam->names[r].size();
        *w++ = '\n';
        lengths_out[r] = bam->lengths[r];
    }
    for (size_t r = 0; r < bam->offsets.size(); ++r) offsets_out[r] = bam->offsets[r];
    return WC_OK;
}

const int32_t *wc_bam_pos(const wc_bam *bam) { return bam ? bam->pos.data() : nullptr; }
const uint8_t *wc_bam_mapq(const wc_bam *bam) { return bam ? bam->mapq.data() : nullptr; }
const uint16_t *wc_bam_flag(const wc_bam *bam) { return bam ? bam->flag.data() : nullptr; }
const int32_t *wc_bam_mate_pos(const wc_bam *bam) { return bam ? bam->mate_pos.data() : nullptr; }

void wc_bam_close(wc_bam *bam) { delete bam; }

}  // extern "C"
