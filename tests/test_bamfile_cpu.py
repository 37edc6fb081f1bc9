"""The host stage of the device BAM reader (csrc/bamfile.cpp: file, BGZF block directory, header) on the block cuts of
tests/test_bamio_cpu.py, and its error codes against the host reader (BamReads) on the same bytes.  Host only: runs
without a GPU."""
import struct

import numpy as np
import pytest

import bam_writer as bw
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

REFS = [("chr1", 50000), ("chrM", 16571), ("2", 40000), ("GL000207.1", 4262), ("chrX", 30000), ("chrY", 9000)]


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


def _blob(data, cuts):
    if cuts == "regular":
        return bw.bgzf(data)
    if cuts == "random":
        return bw.bgzf(data, sorted(np.random.RandomState(3).randint(1, len(data), 400).tolist()))
    if cuts == "tiny":
        return bw.bgzf(data, list(range(7, len(data), 1013)), eof=False)
    return bw.bgzf(data, list(range(1, 200)) + [len(data) - 3, len(data) - 1])


def _block_count(blob):
    at = n = 0
    while at < len(blob):
        at += struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
        n += 1
    return n


@pytest.mark.parametrize("cuts", ["regular", "random", "tiny", "one_block_per_byte_of_header"])
def test_host_stage_reads_directory_and_header(tmp_path, cuts):
    data = bw.plain_bam(REFS, _records())
    blob = _blob(data, cuts)
    path = str(tmp_path / "a.bam")
    open(path, "wb").write(blob)
    with wt.BamFile(path) as f:
        assert f.n_blocks == _block_count(blob)
        assert f.inflated_bytes == len(data)
        assert f.compressed_bytes == len(blob)
        assert f.names == [n for n, _ in REFS] and list(f.lengths) == [l for _, l in REFS]
        assert f.first_record == len(bw.plain_bam(REFS, []))


def test_no_references_and_no_records(tmp_path):
    path = str(tmp_path / "a.bam")
    data = bw.write_bam(path, [], [(-1, -1, 0, 4)])
    with wt.BamFile(path) as f:
        assert f.names == [] and f.first_record == len(bw.plain_bam([], [])) and f.inflated_bytes == len(data)
    data = bw.write_bam(path, REFS, [])
    with wt.BamFile(path) as f:
        assert f.first_record == len(data) == f.inflated_bytes and f.names[2] == "2"


def _code(cls, path):
    with pytest.raises(_lib.WisecondorHipError) as e:
        cls(path)
    assert len(str(e.value)) > 30
    return e.value.code, str(e.value)


def test_host_stage_errors_carry_the_host_readers_codes(tmp_path):
    data = bw.plain_bam(REFS, _records(5, 1500))
    good = bw.bgzf(data, list(range(5000, len(data), 5000)))
    first = struct.unpack("<H", good[16:18])[0] + 1
    path = str(tmp_path / "bad.bam")
    no_bc = bytearray(good)
    no_bc[12:14] = b"XY"                                         # the extra field is there, its BC tag is not
    small = bytearray(good)
    small[first + 16:first + 18] = struct.pack("<H", 20)        # a block size smaller than its own header
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
    }
    for what, (blob, word) in cases.items():
        open(path, "wb").write(blob)
        code, text = _code(wt.BamFile, path)
        want, _ = _code(wt.BamReads, path)
        assert code == want == _lib.E_FORMAT, what
        assert word in text, (what, text)
    missing = str(tmp_path / "missing.bam")
    assert _code(wt.BamFile, missing)[0] == _code(wt.BamReads, missing)[0] == _lib.E_IO
    # an ISIZE beyond 64 KiB
    big = bytearray(good)
    big[first - 4:first] = struct.pack("<I", 70000)
    open(path, "wb").write(bytes(big))
    assert _code(wt.BamFile, path)[0] == _code(wt.BamReads, path)[0] == _lib.E_FORMAT
    # a damaged block among those the header needs: the host stage inflates it, so it reports it
    flipped = bytearray(bw.bgzf(data))
    flipped[40] ^= 0x55
    open(path, "wb").write(bytes(flipped))
    assert _code(wt.BamFile, path)[0] == _code(wt.BamReads, path)[0] == _lib.E_FORMAT
