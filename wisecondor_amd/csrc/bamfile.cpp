// Host stage of the device BAM reader (bamgpu.hip): the whole file into pinned host memory, the BGZF block directory
// (gzip magic, BC field, BSIZE, ISIZE <= 65536), zlib on as many leading blocks as the BAM header needs, the header
// itself (names, lengths, offset of the first record in the inflated stream).  Nothing else is inflated here: the
// compressed bytes are what crosses to the device.  No GPU is needed: without one the buffer is ordinary memory.
// The streamed reader's host stage (wc_bamchunks, below) takes the header from a prefix of the file, then a reader thread
// fills two staging buffers with runs of whole blocks; the file is never held whole.
// The block header rules, the inflate of one block and the BAM header parser are the only ones of the library: the host
// reader (bamio.cpp) uses them through bamfile.h, so the same file gives the same text and code from every reader.
#include <hip/hip_runtime_api.h>
#include <zlib.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
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

int bgzf_block_at(const unsigned char *p, size_t n, size_t at, long long block_no, BgzfBlock &b, size_t &next) {
    if (n - at < 12) { set_error("bam: truncated BGZF block %lld (header cut short)", block_no); return BGZF_CUT; }
    const unsigned char *h = p + at;
    if (h[0] != 31 || h[1] != 139 || h[2] != 8 || !(h[3] & 4)) {
        set_error(block_no ? "bam: damaged BGZF block %lld (no gzip header with an extra field)"
                           : "bam: bad magic: not a BGZF file (block %lld)", block_no);
        return WC_E_FORMAT;
    }
    const size_t xlen = rd16(h + 10);
    if (n - at - 12 < xlen) { set_error("bam: truncated BGZF block %lld (extra field cut short)", block_no); return BGZF_CUT; }
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
        return BGZF_CUT;
    }
    b.in_off = (int64_t)(at + 12 + xlen);
    b.in_len = (int32_t)(rest - 8);
    b.crc = rd32(p + b.in_off + rest - 8);
    b.isize = rd32(p + b.in_off + rest - 4);
    b.pad_ = 0;
    if (b.isize > 65536) { set_error("bam: damaged BGZF block %lld (%u bytes of data announced)", block_no, b.isize); return WC_E_FORMAT; }
    b.out_off = 0;
    next = at + 12 + xlen + (size_t)rest;
    return WC_OK;
}

int bgzf_directory(const unsigned char *p, size_t n, std::vector<BgzfBlock> &blocks, int64_t &total) {
    blocks.clear();
    total = 0;
    size_t at = 0;
    long long block_no = 0;
    while (at < n) {
        BgzfBlock b;
        if (bgzf_block_at(p, n, at, block_no, b, at)) return WC_E_FORMAT;
        b.out_off = total;
        total += b.isize;
        blocks.push_back(b);
        ++block_no;
    }
    return WC_OK;
}

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

int inflate_failed(long long block_no) {
    set_error("bam: damaged BGZF block %lld (inflate or CRC failed)", block_no);
    return WC_E_FORMAT;
}

int header_cut() {
    set_error("bam: truncated: the data ends inside the BAM header");
    return WC_E_FORMAT;
}

long long parse_header(const unsigned char *p, size_t n, std::vector<std::string> &names, std::vector<int64_t> &lengths) {
    if (n >= 4 && memcmp(p, "BAM\1", 4) != 0) {
        set_error("bam: bad magic (the inflated data does not start with BAM\\1)");
        return -1;
    }
    if (n < 12) return 0;
    const int32_t l_text = (int32_t)rd32(p + 4);
    if (l_text < 0) { set_error("bam: negative header text length"); return -1; }
    size_t at = 8 + (size_t)l_text;
    if (n < at + 4) return 0;
    const int32_t n_ref = (int32_t)rd32(p + at);
    at += 4;
    if (n_ref < 0) { set_error("bam: negative reference count"); return -1; }
    names.clear();
    lengths.clear();
    for (int32_t r = 0; r < n_ref; ++r) {
        if (n < at + 4) return 0;
        const int32_t l_name = (int32_t)rd32(p + at);
        if (l_name < 1) { set_error("bam: reference %d has a name of %d bytes", r, l_name); return -1; }
        if (n < at + 4 + (size_t)l_name + 4) return 0;
        names.emplace_back(reinterpret_cast<const char *>(p + at + 4), strnlen(reinterpret_cast<const char *>(p + at + 4), (size_t)l_name));
        lengths.push_back((int64_t)(int32_t)rd32(p + at + 4 + l_name));
        at += 8 + (size_t)l_name;
    }
    return (long long)at;
}

}  // namespace wc

namespace {

const size_t BGZF_MAX_BLOCK = 65536;                // BSIZE has 16 bits

// The header from the file's leading blocks, which are checked and inflated one by one until the header is whole.
// more(raw, have) makes more of the file's leading bytes readable at raw[0 .. have): 1 it did, 0 the file ends at
// `have`, WC_E_IO with a text.
template <class More> int read_header(More more, wc_bamfile &h) {
    std::vector<unsigned char> plain;
    const unsigned char *raw = nullptr;
    size_t have = 0, at = 0;
    bool eof = false;
    long long block_no = 0, first = 0;
    while (first == 0) {
        wc::BgzfBlock b;
        size_t next = 0;
        int rc = wc::BGZF_CUT;
        if (at < have) rc = wc::bgzf_block_at(raw, have, at, block_no, b, next);
        else if (eof) return wc::header_cut();
        if (rc == wc::BGZF_CUT) {
            if (eof) return WC_E_FORMAT;                        // the text of the cut block stands
            const int got = more(raw, have);
            if (got < 0) return got;
            eof = got == 0;
            continue;
        }
        if (rc) return rc;
        const size_t base = plain.size();
        plain.resize(base + b.isize + 1);
        if (!wc::inflate_block(raw, b, plain.data() + base)) return wc::inflate_failed(block_no);
        plain.resize(base + b.isize);
        first = wc::parse_header(plain.data(), plain.size(), h.names, h.lengths);
        if (first < 0) return WC_E_FORMAT;
        at = next;
        ++block_no;
    }
    h.first_record = first;
    h.name_bytes = 0;
    for (const std::string &s : h.names) h.name_bytes += (int64_t)s.size() + 1;
    return WC_OK;
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
    // the header: the whole file is there, and the directory has passed every block header
    return read_header([&](const unsigned char *&raw, size_t &have) {
        if (raw) return 0;
        raw = f.data;
        have = f.size;
        return 1;
    }, f);
}

// ---- the streamed reader's host stage -------------------------------------------------------------------------------
const int64_t STREAM_DEFAULT_CHUNK = 256ll << 20;   // the fastest size of profiles/convert_stream_times.json

// The header from a prefix of the file, read on in steps of four blocks' room.
int read_header_fd(int fd, wc_bamfile &h) {
    std::vector<unsigned char> buf;
    return read_header([&](const unsigned char *&raw, size_t &have) {
        buf.resize(have + 4 * BGZF_MAX_BLOCK);
        raw = buf.data();
        ssize_t got;
        do got = pread(fd, buf.data() + have, buf.size() - have, (off_t)have);
        while (got < 0 && errno == EINTR);
        if (got < 0) {
            wc::set_error("bam: cannot read the file (%s)", strerror(errno));
            return (int)WC_E_IO;
        }
        have += (size_t)got;
        return got ? 1 : 0;
    }, h);
}

}  // namespace

struct wc_bamchunks {
    struct Fill {                       // one staging buffer's chunk, or the reader thread's last word
        std::vector<wc::BgzfBlock> blocks;
        int64_t first_block = 0, bytes = 0, inflated = 0, file_offset = 0;
        bool last = false, end = false;
        int rc = WC_OK;
        std::string error;
    };
    wc_bamfile hdr;                     // the header alone: no data
    int fd = -1;
    int64_t chunk_bytes = 0;
    size_t room = 0;                    // data bytes of one staging buffer; WC_BGZF_PAD more are allocated
    unsigned char *buf[2] = {nullptr, nullptr};
    bool pinned = false;
    Fill fill[2];
    bool full[2] = {false, false};      // under mu: the buffer holds a chunk the caller has not released
    bool stop = false;
    std::mutex mu;
    std::condition_variable cv;
    std::thread reader;
    int64_t taken = 0;                  // the caller's side: chunks handed out,
    int held = -1;                      // the buffer it holds,
    bool done = false;                  // nothing follows
    wc_bamchunks() = default;
    wc_bamchunks(const wc_bamchunks &) = delete;
    wc_bamchunks &operator=(const wc_bamchunks &) = delete;
    ~wc_bamchunks() {
        if (reader.joinable()) {
            {
                std::lock_guard<std::mutex> lk(mu);
                stop = true;
            }
            cv.notify_all();
            reader.join();
        }
        for (unsigned char *b : buf) {
            if (b && pinned) (void)hipHostFree(b);
            else free(b);
        }
        if (fd >= 0) close(fd);
    }
};

namespace {

// The reader thread: fill k goes to buffer k & 1 once the caller has released it.  The bytes behind a fill's chunk (a
// block cut by the end of the read, or whole blocks beyond chunk_bytes) are copied to the front of the next buffer before
// the file is read on; the buffer they come from is not written before the fill after that.
void read_chunks(wc_bamchunks *c) {
    int64_t file_at = 0, chunk_off = 0, block_no = 0;
    size_t left = 0;
    const unsigned char *left_from = nullptr;
    for (int64_t k = 0;; ++k) {
        const int slot = (int)(k & 1);
        {
            std::unique_lock<std::mutex> lk(c->mu);
            c->cv.wait(lk, [&] { return c->stop || !c->full[slot]; });
            if (c->stop) return;
        }
        wc_bamchunks::Fill &f = c->fill[slot];
        f = wc_bamchunks::Fill();
        unsigned char *b = c->buf[slot];
        if (left) memcpy(b, left_from, left);           // left < room: the chunk before took a block or more
        size_t n = left;
        bool eof = false;
        while (n < c->room && !eof && !f.rc) {
            const ssize_t got = pread(c->fd, b + n, c->room - n, (off_t)file_at);
            if (got < 0) {
                if (errno == EINTR) continue;
                f.rc = WC_E_IO;
                f.error = std::string("bam: cannot read the file (") + strerror(errno) + ")";
            } else if (got == 0) {
                eof = true;
            } else {
                n += (size_t)got;
                file_at += got;
            }
        }
        if (!f.rc && !eof) {                            // the buffer is full: does the file end here?
            unsigned char probe;
            ssize_t got;
            do got = pread(c->fd, &probe, 1, (off_t)file_at);
            while (got < 0 && errno == EINTR);
            eof = got == 0;
        }
        memset(b + n, 0, WC_BGZF_PAD);
        if (!f.rc && n == 0) f.end = true;
        size_t at = 0;
        int64_t total = 0;
        while (!f.rc && at < n) {
            // whole blocks while they fit chunk_bytes, and one block at the least
            if (!f.blocks.empty() && (int64_t)at >= c->chunk_bytes) break;
            wc::BgzfBlock blk;
            size_t next = 0;
            const int rc = wc::bgzf_block_at(b, n, at, block_no + (long long)f.blocks.size(), blk, next);
            if (rc == wc::BGZF_CUT && !eof && !f.blocks.empty()) break;     // the next read completes it
            if (rc) {
                // a defect belongs to the chunk its block starts: the blocks before it go out first
                if (!f.blocks.empty()) break;
                f.rc = WC_E_FORMAT;
                f.error = wc_last_error();
                break;
            }
            if (!f.blocks.empty() && (int64_t)next > c->chunk_bytes) break;
            blk.out_off = total;
            total += blk.isize;
            f.blocks.push_back(blk);
            at = next;
        }
        f.bytes = (int64_t)at;
        f.inflated = total;
        f.first_block = block_no;
        f.file_offset = chunk_off;
        block_no += (int64_t)f.blocks.size();
        chunk_off += (int64_t)at;
        left = n - at;
        left_from = b + at;
        f.last = eof && left == 0;
        const bool over = f.rc || f.end || f.last;
        {
            std::lock_guard<std::mutex> lk(c->mu);
            c->full[slot] = true;
        }
        c->cv.notify_all();
        if (over) return;
    }
}

int open_chunks(const char *path, int device, int64_t chunk_bytes, wc_bamchunks &c) {
    c.fd = open(path, O_RDONLY | O_CLOEXEC);
    if (c.fd < 0) { wc::set_error("bam: cannot open %s", path); return WC_E_IO; }
    struct stat st;
    if (fstat(c.fd, &st) != 0 || !S_ISREG(st.st_mode)) { wc::set_error("bam: cannot seek in %s", path); return WC_E_IO; }
    c.hdr.size = (size_t)st.st_size;
    const int rc = read_header_fd(c.fd, c.hdr);
    if (rc) return rc;
    c.chunk_bytes = chunk_bytes > 0 ? chunk_bytes : STREAM_DEFAULT_CHUNK;
    // a read always holds the chunk's blocks and the whole of the block that no longer fits
    c.room = (size_t)std::min<int64_t>(c.chunk_bytes, std::max<int64_t>((int64_t)c.hdr.size, 1)) + BGZF_MAX_BLOCK;
    const size_t cap = c.room + WC_BGZF_PAD;
    const auto t0 = std::chrono::steady_clock::now();
    void *a = nullptr, *b = nullptr;
    if (device >= 0 && hipSetDevice(device) == hipSuccess && hipHostMalloc(&a, cap, hipHostMallocDefault) == hipSuccess) {
        if (hipHostMalloc(&b, cap, hipHostMallocDefault) != hipSuccess) {
            (void)hipHostFree(a);
            wc::set_error("bam: no pinned memory for two staging buffers of %zu bytes", cap);
            return WC_E_LIMIT;
        }
        c.pinned = true;
        c.hdr.pin_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    } else {
        (void)hipGetLastError();
        a = malloc(cap);
        b = malloc(cap);
        if (!a || !b) {
            free(a);
            free(b);
            wc::set_error("bam: no memory for two staging buffers of %zu bytes", cap);
            return WC_E_LIMIT;
        }
    }
    c.buf[0] = static_cast<unsigned char *>(a);
    c.buf[1] = static_cast<unsigned char *>(b);
    c.reader = std::thread(read_chunks, &c);
    return WC_OK;
}

}  // namespace

namespace wc {

int bamchunks_next(wc_bamchunks *it, wc_bamchunk &c) {
    c = wc_bamchunk();
    if (it->held >= 0) {
        {
            std::lock_guard<std::mutex> lk(it->mu);
            it->full[it->held] = false;
        }
        it->cv.notify_all();
        it->held = -1;
    }
    if (it->done) return WC_OK;
    const int slot = (int)(it->taken & 1);
    {
        std::unique_lock<std::mutex> lk(it->mu);
        it->cv.wait(lk, [&] { return it->full[slot]; });
    }
    const wc_bamchunks::Fill &f = it->fill[slot];
    if (f.rc || f.end) {
        it->done = true;
        if (f.rc) set_error("%s", f.error.c_str());
        return f.rc;
    }
    c.data = it->buf[slot];
    c.blocks = f.blocks.data();
    c.n_blocks = (int64_t)f.blocks.size();
    c.first_block = f.first_block;
    c.bytes = f.bytes;
    c.inflated = f.inflated;
    c.file_offset = f.file_offset;
    c.last = f.last;
    it->held = slot;
    ++it->taken;
    it->done = f.last;
    return WC_OK;
}

const wc_bamfile &bamchunks_header(const wc_bamchunks *it) { return it->hdr; }
int64_t bamchunks_host_bytes(const wc_bamchunks *it) { return 2 * (int64_t)(it->room + WC_BGZF_PAD); }
bool bamchunks_pinned(const wc_bamchunks *it) { return it->pinned; }

}  // namespace wc

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

int wc_bamchunks_open(const char *path, int device, int64_t chunk_bytes, wc_bamchunks **out) {
    if (!path || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    *out = nullptr;
    wc_bamchunks *c = nullptr;
    int rc;
    try {
        c = new wc_bamchunks();
        rc = open_chunks(path, device, chunk_bytes, *c);
    } catch (const std::exception &e) {
        wc::set_error("bam: %s", e.what());
        rc = WC_E_LIMIT;
    }
    if (rc != WC_OK) { delete c; return rc; }
    *out = c;
    return WC_OK;
}

int wc_bamchunks_info(const wc_bamchunks *c, int64_t out[8]) {
    if (!c || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    out[0] = (int64_t)c->hdr.names.size();
    out[1] = 0;
    out[2] = 0;
    out[3] = (int64_t)c->hdr.size;
    out[4] = c->hdr.first_record;
    out[5] = c->hdr.name_bytes;
    out[6] = c->pinned ? 1 : 0;
    out[7] = wc::bamchunks_host_bytes(c);
    return WC_OK;
}

int wc_bamchunks_refs(const wc_bamchunks *c, char *names_out, int64_t names_cap, int64_t *lengths_out) {
    if (!c) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    return wc_bamfile_refs(&c->hdr, names_out, names_cap, lengths_out);
}

int wc_bamchunks_next(wc_bamchunks *c, int64_t out[8]) {
    if (!c || !out) { wc::set_error("bam: NULL argument"); return WC_E_ARG; }
    for (int k = 0; k < 8; ++k) out[k] = 0;
    wc_bamchunk ch;
    int rc;
    try {
        rc = wc::bamchunks_next(c, ch);
    } catch (const std::exception &e) {
        wc::set_error("bam: %s", e.what());
        rc = WC_E_LIMIT;
    }
    if (rc || !ch.data) return rc;
    out[0] = 1;
    out[1] = ch.first_block;
    out[2] = ch.n_blocks;
    out[3] = ch.bytes;
    out[4] = ch.inflated;
    out[5] = ch.file_offset;
    out[6] = ch.last ? 1 : 0;
    return WC_OK;
}

void wc_bamchunks_close(wc_bamchunks *c) { delete c; }

int64_t wc_bam_stream_default_chunk(void) { return STREAM_DEFAULT_CHUNK; }

}  // extern "C"
