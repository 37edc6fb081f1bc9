// A stand-alone check of the BAM readers' host code (csrc/bamfile.cpp, csrc/bamio.cpp) for a sanitizer build, no GPU and
// no Python:
//
//   hipcc -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined tools/bamchunks_check.cpp \
//         wisecondor_amd/csrc/bamfile.cpp wisecondor_amd/csrc/bamio.cpp -lz -o bamchunks_check &&
//   ./bamchunks_check FILE.bam CHUNK_BYTES [CHUNK_BYTES ...]
//
// First the host reader (wc_bam_open), which shares its block, inflate, header and record rules with the other two,
// reads the whole file: its names and lengths must be those of the whole-file host stage.
// For every chunk size it walks the chunk iterator to the end and compares each chunk, block by block, with the directory
// of the whole-file host stage (wc_bamfile_open): the same raw-deflate bytes in the staging buffer (so the bytes carried
// from one staging buffer to the next are the file's), the same CRC and ISIZE words, running output offsets, the chunk
// rule (the most whole blocks within CHUNK_BYTES, one at the least) and the header.  Exit status 0 and "ok" per size.
#include <stdarg.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../wisecondor_amd/csrc/bamfile.h"

namespace wc {
static thread_local char g_error[1024] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
}  // namespace wc
extern "C" const char *wc_last_error(void) { return wc::g_error; }

#define REQUIRE(cond)                                                            \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #cond);     \
            return 1;                                                            \
        }                                                                        \
    } while (0)

static int check(const char *path, const wc_bamfile &whole, long long chunk_bytes) {
    wc_bamchunks *it = nullptr;
    if (wc_bamchunks_open(path, -1, chunk_bytes, &it)) {
        fprintf(stderr, "open: %s\n", wc_last_error());
        return 1;
    }
    const wc_bamfile &hdr = wc::bamchunks_header(it);
    REQUIRE(hdr.names == whole.names && hdr.lengths == whole.lengths && hdr.first_record == whole.first_record);
    size_t k = 0;
    long long chunks = 0, file_at = 0;
    bool last_seen = false;
    for (;;) {
        wc_bamchunk c;
        if (wc::bamchunks_next(it, c)) {
            fprintf(stderr, "next: %s\n", wc_last_error());
            return 1;
        }
        if (!c.data) break;
        REQUIRE(!last_seen && c.n_blocks >= 1 && c.first_block == (long long)k && c.file_offset == file_at);
        long long inflated = 0;
        for (long long j = 0; j < c.n_blocks; ++j, ++k) {
            REQUIRE(k < whole.blocks.size());
            const wc::BgzfBlock &a = c.blocks[j], &b = whole.blocks[k];
            REQUIRE(a.in_off + file_at == b.in_off && a.in_len == b.in_len && a.crc == b.crc && a.isize == b.isize);
            REQUIRE(a.out_off == inflated && a.in_off + a.in_len + 8 <= c.bytes);
            REQUIRE(memcmp(c.data + a.in_off, whole.data + b.in_off, (size_t)a.in_len + 8) == 0);
            inflated += a.isize;
        }
        REQUIRE(inflated == c.inflated);
        REQUIRE(c.n_blocks == 1 || c.bytes <= chunk_bytes);
        if (k < whole.blocks.size()) {      // the next block did not fit
            const wc::BgzfBlock &b = whole.blocks[k];
            REQUIRE(b.in_off + b.in_len + 8 - file_at > chunk_bytes);
        }
        file_at += c.bytes;
        ++chunks;
        last_seen = c.last;
    }
    REQUIRE(last_seen && k == whole.blocks.size() && file_at == (long long)whole.size);
    wc_bamchunks_close(it);
    // a second iterator closed half way: the reader thread is stopped while it holds or waits for a buffer
    if (wc_bamchunks_open(path, -1, chunk_bytes, &it)) return 1;
    wc_bamchunk c;
    for (long long j = 0; j < chunks / 2; ++j)
        if (wc::bamchunks_next(it, c)) return 1;
    wc_bamchunks_close(it);
    printf("ok: chunk_bytes %lld, %lld chunks, %zu blocks\n", chunk_bytes, chunks, k);
    return 0;
}

// the host reader's header against the whole-file host stage's; every record of the file goes through the record rule
static int check_host_reader(const char *path, const wc_bamfile &whole) {
    wc_bam *bam = nullptr;
    if (wc_bam_open(path, 4, &bam)) {
        fprintf(stderr, "wc_bam_open: %s\n", wc_last_error());
        return 1;
    }
    int64_t info[8];
    REQUIRE(wc_bam_info(bam, info) == WC_OK);
    REQUIRE(info[0] == (int64_t)whole.names.size() && info[5] == whole.name_bytes);
    std::string names((size_t)info[5], '\0'), want;
    std::vector<int64_t> lengths(whole.names.size()), offsets(whole.names.size() + 1);
    REQUIRE(wc_bam_refs(bam, &names[0], info[5], lengths.data(), offsets.data()) == WC_OK);
    for (const std::string &n : whole.names) want += n + "\n";
    REQUIRE(names == want && lengths == whole.lengths);
    REQUIRE(offsets.back() == info[1] && info[1] > 0);
    printf("ok: host reader, %lld references, %lld placed records\n", (long long)info[0], (long long)info[1]);
    wc_bam_close(bam);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: %s FILE.bam CHUNK_BYTES [CHUNK_BYTES ...]\n", argv[0]);
        return 2;
    }
    wc_bamfile *whole = nullptr;
    if (wc_bamfile_open(argv[1], -1, &whole)) {
        fprintf(stderr, "%s\n", wc_last_error());
        return 1;
    }
    int rc = check_host_reader(argv[1], *whole);
    for (int a = 2; a < argc && !rc; ++a) rc = check(argv[1], *whole, atoll(argv[a]));
    wc_bamfile_close(whole);
    return rc;
}
