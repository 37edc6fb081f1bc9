// What the host stage (bamfile.cpp) hands to the device stage (bamgpu.hip).
#pragma once
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

// The block directory of n BGZF bytes; WC_E_FORMAT with a text on a damaged block header.
int bgzf_directory(const unsigned char *p, size_t n, std::vector<BgzfBlock> &blocks, int64_t &total);

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
