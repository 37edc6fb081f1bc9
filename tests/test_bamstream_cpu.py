"""The host stage of the streamed device BAM reader (csrc/bamfile.cpp, wc_bamchunks): the chunk rule on the block cuts of
tests/test_bamfile_cpu.py, the header across many chunks, the error codes against BamFile, the memory bound of
tests/test_bamstream_gpu.py evaluated on the CPU, and the -stream / -chunk options.  Host only: runs without a GPU."""
import struct

import numpy as np
import pytest

import bam_writer as bw
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

REFS = [("chr1", 50000), ("chrM", 16571), ("2", 40000), ("GL000207.1", 4262), ("chrX", 30000), ("chrY", 9000)]
CUTS = ["regular", "random", "tiny", "one_block_per_byte_of_header"]
BGZF_PAD = 64                   # WC_BGZF_PAD of csrc/bamfile.h
SEG = 65536                     # wc_bam_chain_segment(), asserted on the GPU


def _records(seed=1, n=3000):
    rng = np.random.RandomState(seed)
    ids, pos, mapq = [], [], []
    for r, (_, length) in enumerate(REFS):
        if r == 3:
            continue
        k = 1 if r == 5 else n + 17 * r
        ids.append(r)
        pos.append(np.sort(rng.randint(0, length, k)))
        mapq.append(rng.choice([0, 1, 30, 60, 255], k))
    return bw.records_of(ids, pos, mapq, unplaced=5)


def blob_of(data, cuts):
    if cuts == "regular":
        return bw.bgzf(data)
    if cuts == "random":
        return bw.bgzf(data, sorted(np.random.RandomState(3).randint(1, len(data), 400).tolist()))
    if cuts == "tiny":
        return bw.bgzf(data, list(range(7, len(data), 1013)), eof=False)
    return bw.bgzf(data, list(range(1, 200)) + [len(data) - 3, len(data) - 1])


def block_sizes(blob):
    """(compressed bytes, ISIZE) of every BGZF block, from the block headers."""
    at, out = 0, []
    while at < len(blob):
        size = struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
        out.append((size, struct.unpack("<I", blob[at + size - 4:at + size])[0]))
        at += size
    return out


def chunking(blocks, chunk):
    """The chunk rule restated: [(blocks, compressed bytes, inflated bytes)]."""
    out, k = [], 0
    while k < len(blocks):
        n, c, t = 1, blocks[k][0], blocks[k][1]
        while k + n < len(blocks) and c + blocks[k + n][0] <= chunk:
            c += blocks[k + n][0]
            t += blocks[k + n][1]
            n += 1
        out.append((n, c, t))
        k += n
    return out


def working_need(c, t, n_blocks, n_ref):
    """The whole-file reader's documented need (csrc/bamgpu.hip, open_dev) for c compressed and t inflated bytes without
    its per-record output term: compressed bytes and pad, directory and status, inflated bytes, 2 bytes of map per
    inflated byte in whole segments, three words per segment, the offsets, 4096."""
    n_seg = (t + SEG - 1) // SEG
    return c + BGZF_PAD + n_blocks * (32 + 4) + t + 64 + 2 * n_seg * SEG + 16 * n_seg + 8 * (n_ref + 1) + 4096


def working_bound(c, t, carry, n_blocks, n_ref):
    """The bound on the streamed reader's peak device working bytes: twice (double buffering) the need of the largest
    chunk with the largest carry in front of it, plus 64 KiB."""
    return 2 * working_need(c, t + carry, n_blocks, n_ref) + 65536


def big_records(n_per_ref):
    rng = np.random.RandomState(5)
    refs = [("chr%d" % (c + 1), 2000000) for c in range(4)]
    recs = []
    for c in range(4):
        p = np.sort(rng.randint(0, 2000000, n_per_ref))
        recs += list(zip([c] * n_per_ref, p.tolist(), rng.randint(0, 61, n_per_ref).tolist(), [0] * n_per_ref))
    return refs, recs


@pytest.mark.parametrize("chunk", [1, 4096, 70000, 1 << 30])
@pytest.mark.parametrize("cuts", CUTS)
def test_chunks_partition_the_blocks_and_the_header_equals_bamfiles(tmp_path, cuts, chunk):
    data = bw.plain_bam(REFS, _records())
    blob = blob_of(data, cuts)
    path = str(tmp_path / "a.bam")
    open(path, "wb").write(blob)
    blocks = block_sizes(blob)
    want = chunking(blocks, chunk)
    if chunk == 1:
        assert len(want) == len(blocks)
    if cuts == "one_block_per_byte_of_header" and chunk == 1:
        assert len(want) > 200                          # the header alone spans 200 one-block chunks
    with wt.BamFile(path, device=-1) as f, wt.BamChunks(path, device=-1, chunk=chunk) as c:
        assert c.names == f.names and list(c.lengths) == list(f.lengths) and c.first_record == f.first_record
        assert c.compressed_bytes == f.compressed_bytes == len(blob)
        assert c.host_bytes <= 2 * (min(chunk, len(blob)) + 65536 + BGZF_PAD) and not c.pinned
        got = list(c)
        assert [(g["blocks"], g["compressed_bytes"], g["inflated_bytes"]) for g in got] == want
        assert [g["first_block"] for g in got] == np.concatenate([[0], np.cumsum([w[0] for w in want])[:-1]]).tolist()
        assert [g["file_offset"] for g in got] == np.concatenate([[0], np.cumsum([w[1] for w in want])[:-1]]).tolist()
        assert [g["last"] for g in got] == [False] * (len(got) - 1) + [True]
        assert sum(g["blocks"] for g in got) == f.n_blocks == len(blocks)
        assert sum(g["compressed_bytes"] for g in got) == f.compressed_bytes
        assert sum(g["inflated_bytes"] for g in got) == f.inflated_bytes == len(data)
        assert list(c) == []                            # behind the last chunk: nothing, again and again


def _code(open_it, path):
    with pytest.raises(_lib.WisecondorHipError) as e:
        open_it(path)
    assert len(str(e.value)) > 30
    return e.value.code, str(e.value)


def _walk(chunk, seen):
    def open_it(path):
        with wt.BamChunks(path, device=-1, chunk=chunk) as c:
            for g in c:
                seen.append(g)
    return open_it


@pytest.mark.parametrize("chunk", [1, 4096, 1 << 30])
def test_errors_carry_bamfiles_codes(tmp_path, chunk):
    data = bw.plain_bam(REFS, _records(5, 1500))
    good = bw.bgzf(data, list(range(5000, len(data), 5000)))
    first = struct.unpack("<H", good[16:18])[0] + 1
    path = str(tmp_path / "bad.bam")
    no_bc = bytearray(good)
    no_bc[12:14] = b"XY"
    small = bytearray(good)
    small[first + 16:first + 18] = struct.pack("<H", 20)
    big = bytearray(good)
    big[first - 4:first] = struct.pack("<I", 70000)
    flipped = bytearray(bw.bgzf(data))
    flipped[40] ^= 0x55
    cases = {
        "not BGZF": (b"not a bam file at all, just some text that is long enough", "magic"),
        "empty file: the data ends inside the header": (b"", "header"),
        "data ends inside the header": (bw.bgzf(data[:40]), "header"),
        "bad BAM magic": (bw.bgzf(b"SAM\x01" + data[4:]), "magic"),
        "truncated inside a block": (good[:first + 100], "truncated"),
        "truncated inside a block header": (good[:first + 7], "truncated"),
        "unusable BC field": (bytes(no_bc), "BC"),
        "BSIZE below the header": (bytes(small), "BC"),
        "damaged second gzip magic": (good[:first] + b"\x00" + good[first + 1:], "gzip"),
        "an ISIZE beyond 64 KiB": (bytes(big), "announced"),
        "a damaged block among those the header needs": (bytes(flipped), "inflate"),
    }
    for what, (blob, word) in cases.items():
        open(path, "wb").write(blob)
        seen = []
        code, text = _code(_walk(chunk, seen), path)
        want, want_text = _code(lambda p: wt.BamFile(p, device=-1), path)
        assert code == want == _lib.E_FORMAT, what
        assert word in text, (what, text)
        if what in ("truncated inside a block", "damaged second gzip magic"):
            assert text == want_text                    # the file's block number, not the chunk's
            if chunk < (1 << 30):
                assert len(seen) == 1 and seen[0]["blocks"] == 1, what      # the defect lies in the second chunk
    missing = str(tmp_path / "missing.bam")
    assert _code(_walk(chunk, []), missing)[0] == _code(lambda p: wt.BamFile(p, device=-1), missing)[0] == _lib.E_IO


def test_the_memory_bound_of_the_gpu_test_evaluates_on_the_cpu(tmp_path):
    """tests/test_bamstream_gpu.py holds the streamed reader's peak device working bytes against working_bound() of the
    chunking recomputed here; the inputs stay inside it by construction: the bound is finite, grows with the chunk
    alone, and the two files' largest chunks are of one size although one file is four times the other."""
    chunk = 262144
    bounds = []
    for n in (12500, 50000):
        refs, recs = big_records(n)
        path = str(tmp_path / "a.bam")
        bw.write_bam(path, refs, recs)
        blob = open(path, "rb").read()
        want = chunking(block_sizes(blob), chunk)
        with wt.BamChunks(path, device=-1, chunk=chunk) as c:
            got = [(g["blocks"], g["compressed_bytes"], g["inflated_bytes"]) for g in c]
        assert got == want and len(want) >= 2
        c_max, t_max, b_max = max(w[1] for w in want), max(w[2] for w in want), max(w[0] for w in want)
        assert c_max <= chunk
        # a carry of this writer's records (below 1 000 bytes) moves t into no other chain segment: the GPU test rounds
        # t + carry up to whole segments on both sides of its comparison of the two files
        assert (t_max + 1000 + SEG - 1) // SEG == (t_max + SEG - 1) // SEG
        carry = 65536                                   # no record of this writer is longer
        bounds.append(working_bound(c_max, t_max, carry, b_max, len(refs)))
        assert bounds[-1] < 2 * (chunk + 3 * (t_max + carry + SEG)) + 3 * 65536
    assert len(blob) > 4 * chunk
    assert abs(bounds[1] - bounds[0]) < 0.25 * bounds[0]     # not four times: the file's size is not in it


def test_stream_and_chunk_stay_out_of_the_namespace_unless_given():
    from wisecondor_amd import wisecondor as wc
    parser = wc.buildParser()
    args = parser.parse_args(["convert", "in.bam", "out.npz"])
    assert not hasattr(args, "stream") and not hasattr(args, "chunk")
    args = parser.parse_args(["convert", "in.bam", "out.npz", "-stream", "-chunk", "65536"])
    assert args.stream is True and args.chunk == 65536
    args = parser.parse_args(["convertbatch", "a.bam", "b.bam", "outdir"])
    assert not hasattr(args, "stream") and not hasattr(args, "chunk")
    args = parser.parse_args(["convertbatch", "a.bam", "b.bam", "outdir", "-stream"])
    assert args.stream is True and not hasattr(args, "chunk")
    args = parser.parse_args(["convertbatch", "a.bam", "outdir", "-chunk", "4096", "-stream"])
    assert args.stream is True and args.chunk == 4096


def test_chunk_without_stream_is_an_error_not_an_ignored_option(monkeypatch):
    from wisecondor_amd import wisecondor as wc
    parser = wc.buildParser()
    for argv in (["convert", "in.bam", "out.npz"], ["convertbatch", "a.bam", "outdir"]):
        with pytest.raises(ValueError, match="-stream"):
            wc._convert_streamed(parser.parse_args(argv + ["-chunk", "4096"]))
        assert wc._convert_streamed(parser.parse_args(argv + ["-chunk", "4096", "-stream"])) is True
        assert wc._convert_streamed(parser.parse_args(argv)) is False
    monkeypatch.setattr(wt, "CONVERT_READER", "stream")
    assert wc._convert_streamed(parser.parse_args(["convert", "in.bam", "out.npz", "-chunk", "4096"])) is True


def test_the_default_reader_is_unchanged_and_the_default_chunk_is_the_librarys():
    assert wt.CONVERT_READER == "device" and wt.BAM_STREAM_CHUNK == 0
    assert (8 << 20) <= _lib.load().wc_bam_stream_default_chunk() <= (256 << 20)
