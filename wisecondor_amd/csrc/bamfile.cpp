// Host stage of the device BAM reader (bamgpu.hip): the whole file into pinned host memory, the BGZF block directory
// (the header checks of bamio.cpp's read_bam: gzip magic, BC field, BSIZE, ISIZE <= 65536), zlib on as many leading
// blocks as the BAM header needs, the header itself (names, lengths, offset of the first record in the inflated
// stream).  Nothing else is inflated here: the compressed bytes are what crosses to the device.  Errors carry the codes
// wc_bam_open returns for the same file.  No GPU is needed: without one the buffer is ordinary memory.
#include <hip/hip_runtime_api.h>
#include <zlib.h>

#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bamfile.h"

namespace wc {
void set_error(const char *fmt, ...);

namespace {
inline uint16_t rd16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t rd32(const unsigned char *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
}  // namespace

int bgzf_directory(const unsigned char *p, size_t n, std::vector<BgzfBlock> &blocks, int64_t &total) {
    blocks.clear();
    total = 0;
    size_t at = 0;
    long long block_no = 0;
    while (at < n) {
        if (n - at < 12) { set_error("bam: truncated BGZF block %lld (header cut short)", block_no); return WC_E_FORMAT; }
        const unsigned char *h = p + at;
        if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) {
            set_error(block_no ? "bam: damaged BGZF block %lld (no gzip header with an extra field)"
                               : "bam: bad magic: not a BGZF file (block %lld)", block_no);
            return WC_E_FORMAT;
        }
        const size_t xlen = rd16(h + 10);
        if (n - at - 12 < xlen) { set_error("bam: truncated BGZF block %lld (extra field cut short)", block_no); return WC_E_FORMAT; }
        const unsigned char *x = h + 12;
        long bsize = -1;
        for (size_t q = 0; q + 4 <= xlen;) {
            const size_t slen = rd16(x + q + 2);
            if (x[q] == 'B' && x[q + 1] == 'C' && slen == 2 && q + 6 <= xlen) bsize = rd16(x + q + 4);
            q += 4 + slen;
        }
        const long rest = bsize + 1 - 12 - (long)xlen;
        if (bsize < 0 || rest < 8) { set_error("bam: damaged BGZF block %lld (no usable BC size field)", block_no); return WC_E_FORMAT; }
        if (n - at - 12 - xlen < (size_t)rest) {
            set_error("bam: truncated BGZF block %lld (%ld bytes announced)", block_no, rest);
            return WC_E_FORMAT;
        }
        BgzfBlock b;
        b.in_off = (int64_t)(at + 12 + xlen);
        b.in_len = (int32_t)(rest - 8);
        b.crc = rd32(p + b.in_off + rest - 8);
        b.isize = rd32(p + b.in_off + rest - 4);
        if (b.isize > 65536) { set_error("bam: damaged BGZF block %lld (%u bytes of data announced)", block_no, b.isize); return WC_E_FORMAT; }
        b.out_off = total;
        total += b.isize;
        blocks.push_back(b);
        at += 12 + xlen + (size_t)rest;
        ++block_no;
    }
    return WC_OK;
}

}  // namespace wc

namespace {

using wc::rd32;

bool inflate_block(const unsigned char *in, const wc::BgzfBlock &b, unsigned char *out) {
    unsigned char dummy = 0;
    z_stream zs;
    memset(&zs, 0, sizeof(zs));
    if (inflateInit2(&zs, -15) != Z_OK) return false;
    zs.next_in = const_cast<unsigned char *>(in + b.in_off);
    zs.avail_in = (uInt)b.in_len;
    zs.next_out = b.isize ? out : &dummy;
    zs.avail_out = b.isize ? b.isize : 1;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.total_out == b.isize;
    inflateEnd(&zs);
    if (!ok) return false;
    return (uint32_t)crc32(crc32(0L, Z_NULL, 0), out, b.isize) == b.crc || (b.isize == 0 && b.crc == 0);
}

// The BAM header from the first n inflated bytes: > 0 the offset of the first record, 0 more bytes are needed,
// < 0 an error (text set).  The checks and texts of bamio.cpp's Parser::feed.
long long parse_header(const unsigned char *p, size_t n, wc_bamfile &f) {
    if (n >= 4 && memcmp(p, "BAM\1", 4) != 0) {
        wc::set_error("bam: bad magic (the inflated data does not start with BAM\\1)");
        return -1;
    }
    if (n < 12) return 0;
    const int32_t l_text = (int32_t)rd32(p + 4);
    if (l_text < 0) { wc::set_error("bam: negative header text length"); return -1; }
    size_t at = 8 + (size_t)l_text;
    if (n < at + 4) return 0;
    const int32_t n_ref = (int32_t)rd32(p + at);
    at += 4;
    if (n_ref < 0) { wc::set_error("bam: negative reference count"); return -1; }
    f.names.clear();
    f.lengths.clear();
    for (int32_t r = 0; r < n_ref; ++r) {
        if (n < at + 4) return 0;
        const int32_t l_name = (int32_t)rd32(p + at);
        if (l_name < 1) { wc::set_error("bam: reference %d has a name of %d bytes", r, l_name); return -1; }
        if (n < at + 4 + (size_t)l_name + 4) return 0;
        f.names.emplace_back(reinterpret_cast<const char *>(p + at + 4), strnlen(reinterpret_cast<const char *>(p + at + 4), (size_t)l_name));
        f.lengths.push_back((int64_t)(int32_t)rd32(p + at + 4 + l_name));
        at += 8 + (size_t)l_name;
    }
    return (long long)at;
}

int open_file(const char *path, int device, wc_bamfile &f) {
    FILE *fp = fopen(path, "rb");
    if (!fp) { wc::set_error("bam: cannot open %s", path); return WC_E_IO; }
    struct Closer { FILE *f; ~Closer() { fclose(f); } } closer{fp};
    if (fseek(fp, 0, SEEK_END) != 0) { wc::set_error("bam: cannot seek in %s", path); return WC_E_IO; }
    const long long size = ftell(fp);
    if (size < 0 || fseek(fp, 0, SEEK_SET) != 0) { wc::set_error("bam: cannot seek in %s", path); return WC_E_IO; }
    f.size = (size_t)size;
    const size_t cap = f.size + WC_BGZF_PAD;
    void *mem = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    // pinned against the device that will read it (this may be a read-ahead thread with no device chosen yet)
    if (device >= 0 && hipSetDevice(device) == hipSuccess && hipHostMalloc(&mem, cap, hipHostMallocDefault) == hipSuccess) {
        f.pinned = true;
        f.pin_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    } else {
        (void)hipGetLastError();        // no device: ordinary memory serves the host stage alone
        mem = malloc(cap);
        if (!mem) { wc::set_error("bam: no memory for the %zu bytes of %s", cap, path); return WC_E_LIMIT; }
    }
    f.data = static_cast<unsigned char *>(mem);
    if (f.size && fread(f.data, 1, f.size, fp) != f.size) { wc::set_error("bam: cannot read %s", path); return WC_E_IO; }
    memset(f.data + f.size, 0, WC_BGZF_PAD);
    int rc = wc::bgzf_directory(f.data, f.size, f.blocks, f.total);
    if (rc) return rc;
    // the header: leading blocks only
    std::vector<unsigned char> plain;
    long long first = 0;
    for (size_t k = 0; k < f.blocks.size() && first == 0; ++k) {
        const wc::BgzfBlock &b = f.blocks[k];
        const size_t base = plain.size();
        plain.resize(base + b.isize + 1);
        if (!inflate_block(f.data, b, plain.data() + base)) {
            wc::set_error("bam: damaged BGZF block %lld (inflate or CRC failed)", (long long)k);
            return WC_E_FORMAT;
        }
        plain.resize(base + b.isize);
        first = parse_header(plain.data(), plain.size(), f);
        if (first < 0) return WC_E_FORMAT;
    }
    if (first == 0) { wc::set_error("bam: truncated: the data ends inside the BAM header"); return WC_E_FORMAT; }
    f.first_record = first;
    f.name_bytes = 0;
    for (const std::string &s : f.names) f.name_bytes += (int64_t)s.size() + 1;
    return WC_OK;
}

}  // namespace

wc_bamfile::~wc_bamfile() {
    if (data && pinned) (void)hipHostFree(data);
    else free(data);
}

extern "C" {

int wc_bamfile_open(const char *path, int device, wc_bamfile **out) {
    if (!path || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    *out = nullptr;
    wc_bamfile *f = nullptr;
    int rc;
    try {
        f = new wc_bamfile();
        rc = open_file(path, device, *f);
    } catch (const std::exception &e) {
        wc::set_error("bam: %s", e.what());
        rc = WC_E_LIMIT;
    }
    if (rc != WC_OK) { delete f; return rc; }
    *out = f;
    return WC_OK;
}

int wc_bamfile_info(const wc_bamfile *f, int64_t out[8]) {
    if (!f || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    out[0] = (int64_t)f->names.size();
    out[1] = (int64_t)f->blocks.size();
    out[2] = f->total;
    out[3] = (int64_t)f->size;
    out[4] = f->first_record;
    out[5] = f->name_bytes;
    out[6] = f->pinned ? 1 : 0;
    out[7] = f->pin_us;
    return WC_OK;
}

int wc_bamfile_refs(const wc_bamfile *f, char *names_out, int64_t names_cap, int64_t *lengths_out) {
    if (!f || !names_out || !lengths_out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    if (names_cap < f->name_bytes) { wc::set_error("bam: %lld bytes of names, room for %lld", (long long)f->name_bytes, (long long)names_cap); return WC_E_ARG; }
    char *w = names_out;
    for (size_t r = 0; r < f->names.size(); ++r) {
        memcpy(w, f->names[r].data(), f->names[r].size());
        w += f->names[r].size();
        *w++ = '\n';
        lengths_out[r] = f->lengths[r];
    }
    return WC_OK;
}

void wc_bamfile_close(wc_bamfile *f) { delete f; }

}  // extern "C"
