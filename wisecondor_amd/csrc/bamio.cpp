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
// The file is read in rounds of WC_BAM_CHUNK blocks: compressed bytes in, blocks inflated in parallel into one buffer,
// records parsed from it, the unfinished tail of the buffer carried to the front of the next round.  Errors, never
// crashes: every length is checked against the bytes that are there.  What a valid block, header and record is, is said
// in bamfile.h / bamfile.cpp for all readers; here are the file, the thread pool and the order check.  No GPU code in
// this file.
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "bamfile.h"

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
const size_t WC_BAM_SLAB = 4 << 20; // bytes asked of the file at a time

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
            const long long first = wc::parse_header(p, n, b.names, b.lengths);
            if (first < 0) return fail(WC_E_FORMAT);
            if (first == 0) return 0;
            at = (size_t)first;
            b.offsets.assign(b.names.size() + 1, 0);
            header_done = true;
        }
        const int32_t n_ref = (int32_t)b.names.size();
        for (;;) {
            wc::BamRecord rec;
            const int bad = wc::bam_record(p + at, (long long)(n - at), n_ref, rec);
            if (bad == wc::BAM_R_TRUNC) break;          // the next round brings the rest, or read_bam reports the left-over
            if (bad != wc::BAM_R_OK) {
                if (bad == wc::BAM_R_BS)
                    wc::set_error("bam: record %lld has block_size %d, below its 32 fixed bytes", (long long)records, rec.block_size);
                else if (bad == wc::BAM_R_FIELDS)
                    wc::set_error("bam: the fields of record %lld overrun its block_size (%lld > %d)", (long long)records,
                                  (long long)rec.need, rec.block_size);
                else
                    wc::set_error("bam: record %lld names reference %d of %d", (long long)records, rec.ref, n_ref);
                return fail(WC_E_FORMAT);
            }
            const int32_t ref = rec.ref, ps = rec.pos;
            const unsigned flag = rec.flag;
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
                b.mapq.push_back(rec.mapq);
                b.flag.push_back((uint16_t)flag);
                b.mate_pos.push_back(rec.mate_pos);
                ++b.offsets[(size_t)ref + 1];
            }
            ++records;
            at += 4 + (size_t)rec.block_size;
        }
        return (long long)at;
    }
};

int read_bam(const char *path, int n_threads, wc_bam &bam) {
    FILE *f = fopen(path, "rb");
    if (!f) { wc::set_error("bam: cannot open %s", path); return WC_E_IO; }
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{f};
    std::vector<unsigned char> comp, plain;
    std::vector<wc::BgzfBlock> blocks;
    Parser parser(bam);
    size_t have = 0;            // file bytes at the front of `comp` that no block has taken yet
    size_t left = 0;            // unparsed bytes at the front of `plain`
    long long block_no = 0;
    bool eof = false;
    while (!eof || have) {
        blocks.clear();
        size_t out_bytes = left, at = 0;
        while ((int)blocks.size() < WC_BAM_CHUNK && (at < have || !eof)) {
            wc::BgzfBlock b;
            size_t next = 0;
            const int rc = at < have ? wc::bgzf_block_at(comp.data(), have, at, block_no, b, next) : (int)wc::BGZF_CUT;
            if (rc == wc::BGZF_CUT && !eof) {           // fread, not pread: the path may be one that cannot seek
                if (comp.size() < have + WC_BAM_SLAB) comp.resize(have + WC_BAM_SLAB);
                const size_t got = fread(comp.data() + have, 1, WC_BAM_SLAB, f);
                have += got;
                eof = got < WC_BAM_SLAB;
                continue;
            }
            if (rc) return WC_E_FORMAT;
            b.out_off = (int64_t)out_bytes;
            out_bytes += b.isize;
            blocks.push_back(b);
            at = next;
            ++block_no;
        }
        plain.resize(out_bytes + 1);
        std::atomic<int> bad(-1);
        run_pool((int)blocks.size(), n_threads, [&](int i) {
            if (!wc::inflate_block(comp.data(), blocks[i], plain.data() + blocks[i].out_off)) {
                int none = -1;
                bad.compare_exchange_strong(none, i);
            }
        });
        if (bad.load() >= 0) return wc::inflate_failed(block_no - (long long)blocks.size() + bad.load());
        const long long used = parser.feed(plain.data(), out_bytes);
        if (used < 0) return parser.rc;
        left = out_bytes - (size_t)used;
        if (used && left) memmove(plain.data(), plain.data() + used, left);
        have -= at;
        if (at && have) memmove(comp.data(), comp.data() + at, have);
    }
    if (!parser.header_done) return wc::header_cut();
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
