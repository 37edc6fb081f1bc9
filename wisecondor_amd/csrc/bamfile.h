// What the host stage (bamfile.cpp) hands to the device stage (bamgpu.hip), and the rules of the format that the three
// readers share: the BGZF block header, one block's inflate, the BAM header (bamfile.cpp) and the record (below).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/wisecondor_hip.h"

#define WC_BGZF_PAD 64      // zero bytes behind the compressed data: the decoder's aligned refill may read past a block

namespace wc {

struct BgzfBlock {          // one BGZF block: its raw-deflate bytes and where its data goes (uploaded as it is)
    int64_t in_off, out_off;
    int32_t in_len;
    uint32_t crc, isize;
    uint32_t pad_;
};

// One BGZF block header at p + at of n bytes: WC_OK (b filled, in_off counted from p, out_off 0; next: the offset behind
// the block), WC_E_FORMAT, or BGZF_CUT where the n bytes end inside the block (the text is set all the same: at the end of
// a file that is the error).
enum { BGZF_CUT = 1 };
int bgzf_block_at(const unsigned char *p, size_t n, size_t at, long long block_no, BgzfBlock &b, size_t &next);

// The block directory of n BGZF bytes; WC_E_FORMAT with a text on a damaged block header.
int bgzf_directory(const unsigned char *p, size_t n, std::vector<BgzfBlock> &blocks, int64_t &total);

// zlib on block b of the BGZF bytes at `in`, its isize bytes to `out` (one byte more is writable); false: inflate or CRC failed.
bool inflate_block(const unsigned char *in, const BgzfBlock &b, unsigned char *out);
int inflate_failed(long long block_no);     // its text for the file's block block_no (the calling thread's); WC_E_FORMAT

// The BAM header from the first n inflated bytes: > 0 the offset of the first record (names and lengths filled), 0 more
// bytes are needed, < 0 an error (text set).
long long parse_header(const unsigned char *p, size_t n, std::vector<std::string> &names, std::vector<int64_t> &lengths);
int header_cut();                           // the text of a file whose data end inside the header; WC_E_FORMAT

// ---- the record rule, for the device walk and the host reader alike ---------------------------------------------------
#if defined(__HIP__)
#define WC_BAM_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define WC_BAM_HD inline
#endif

enum { BAM_R_OK = -1, BAM_R_TRUNC = 0, BAM_R_BS = 1, BAM_R_FIELDS = 2, BAM_R_REF = 3 };

struct BamRecord {
    int32_t block_size, ref, pos, mate_pos;
    uint32_t flag;
    uint8_t mapq;
    int64_t need;           // the bytes its fixed part, name, CIGAR, sequence and qualities take
};

WC_BAM_HD uint32_t bam_ld16(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
WC_BAM_HD uint32_t bam_ld32(const unsigned char *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The record whose block_size word is at p, `avail` bytes readable from there, n_ref references in the header: BAM_R_OK
// and its fields, or the first defect.  BAM_R_TRUNC: the record, its block_size word included, overruns the bytes (the
// caller knows whether more will come).  Nothing beyond p + avail is read.
WC_BAM_HD int bam_record(const unsigned char *p, long long avail, int n_ref, BamRecord &f) {
    if (avail < 4) return BAM_R_TRUNC;
    f.block_size = (int32_t)bam_ld32(p);
    if (f.block_size < 32) return BAM_R_BS;
    if (avail - 4 < (long long)f.block_size) return BAM_R_TRUNC;
    const unsigned char *r = p + 4;
    const int32_t l_seq = (int32_t)bam_ld32(r + 16);
    f.ref = (int32_t)bam_ld32(r);
    f.flag = bam_ld16(r + 14);
    f.need = 32 + (int64_t)r[8] + 4 * (int64_t)bam_ld16(r + 12) + ((int64_t)l_seq + 1) / 2 + (int64_t)l_seq;
    if (l_seq < 0 || f.need > (int64_t)f.block_size) return BAM_R_FIELDS;
    if (f.ref >= n_ref) return BAM_R_REF;
    f.pos = (int32_t)bam_ld32(r + 4);
    f.mapq = r[9];
    f.mate_pos = (int32_t)bam_ld32(r + 24);
    return BAM_R_OK;
}

}  // namespace wc

struct wc_bamfile {
    unsigned char *data = nullptr;      // size + WC_BGZF_PAD bytes, pinned when a device is there
    size_t size = 0;
    bool pinned = false;
    int64_t pin_us = 0;                 // microseconds the pinned allocation took
    std::vector<wc::BgzfBlock> blocks;
    int64_t total = 0;                  // sum of ISIZE
    int64_t first_record = 0, name_bytes = 0;
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    wc_bamfile() = default;
    wc_bamfile(const wc_bamfile &) = delete;
    wc_bamfile &operator=(const wc_bamfile &) = delete;
    ~wc_bamfile();
};

// One chunk of the streamed reader (wc_bamchunks_next): a run of whole BGZF blocks in a staging buffer.  The directory's
// in_off counts from `data`, its out_off from the chunk's first inflated byte.  Valid until the next call of next().
struct wc_bamchunk {
    const unsigned char *data = nullptr;        // bytes + WC_BGZF_PAD readable, the pad zeroed
    const wc::BgzfBlock *blocks = nullptr;
    int64_t n_blocks = 0, first_block = 0;      // first_block: the file's number of blocks[0]
    int64_t bytes = 0, inflated = 0;            // compressed bytes of the chunk (whole blocks), the sum of their ISIZE
    int64_t file_offset = 0;
    bool last = false;                          // the file ends with this chunk
};

namespace wc {
// The C++ face of wc_bamchunks_next for the device stage: WC_OK and c.data == nullptr behind the last chunk.
int bamchunks_next(wc_bamchunks *it, wc_bamchunk &c);
const wc_bamfile &bamchunks_header(const wc_bamchunks *it);     // names, lengths, first_record, name_bytes (no data)
int64_t bamchunks_host_bytes(const wc_bamchunks *it);           // of the two staging buffers
bool bamchunks_pinned(const wc_bamchunks *it);
}  // namespace wc
