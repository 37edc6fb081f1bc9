"""The native BAM reader (csrc/bamio.cpp) against a BAM writer of the test's own (tests/bam_writer.py): what was
written is what is read, whatever the BGZF block cuts and the thread count; every damaged copy is an error with a
text, never a crash.  Host only: runs without a GPU."""
import struct

import numpy as np
import pytest

import bam_writer as bw
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

REFS = [("chr1", 50000), ("chrM", 16571), ("2", 40000), ("GL000207.1", 4262), ("chrX", 30000), ("chrY", 9000)]


def _reads(seed, n=3000):
    rng = np.random.RandomState(seed)
    ids, pos, mapq = [], [], []
    for r, (_, length) in enumerate(REFS):
        if r == 3:
            continue                                    # a reference without reads
        k = 1 if r == 5 else n + 17 * r
        ids.append(r)
        pos.append(np.sort(rng.randint(0, length, k)))
        mapq.append(rng.choice([0, 1, 30, 60, 255], k))
    return ids, pos, mapq


def _check(bam, ids, pos, mapq, unplaced):
    assert bam.names == [n for n, _ in REFS] and list(bam.lengths) == [l for _, l in REFS]
    for r in range(len(REFS)):
        a, b = int(bam.offsets[r]), int(bam.offsets[r + 1])
        if r in ids:
            i = ids.index(r)
            assert np.array_equal(bam.pos[a:b], pos[i]) and np.array_equal(bam.mapq[a:b], mapq[i])
        else:
            assert a == b
    assert bam.pos.dtype == np.int32 and bam.mapq.dtype == np.uint8
    recs = bw.records_of(ids, pos, mapq, unplaced)
    assert bam.no_coordinate == unplaced
    assert bam.unmapped == sum(1 for r in recs if r[3] & 4)
    assert bam.mapped == sum(1 for r in recs if r[0] >= 0 and not r[3] & 4)


@pytest.mark.parametrize("cuts", ["regular", "random", "tiny", "one_block_per_byte_of_header"])
def test_reader_returns_what_was_written(tmp_path, cuts):
    ids, pos, mapq = _reads(1)
    recs = bw.records_of(ids, pos, mapq, unplaced=5)
    path = str(tmp_path / "a.bam")
    data = bw.plain_bam(REFS, recs)
    if cuts == "regular":
        blob = bw.bgzf(data)
    elif cuts == "random":
        blob = bw.bgzf(data, sorted(np.random.RandomState(3).randint(1, len(data), 400).tolist()))
    elif cuts == "tiny":
        blob = bw.bgzf(data, list(range(7, len(data), 1013)), eof=False)       # a missing EOF block is accepted
    else:
        blob = bw.bgzf(data, list(range(1, 200)) + [len(data) - 3, len(data) - 1])
    open(path, "wb").write(blob)
    with wt.BamReads(path, threads=3) as bam:
        _check(bam, ids, pos, mapq, 5)


def test_thread_counts_give_equal_output(tmp_path):
    ids, pos, mapq = _reads(2, n=20000)
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, REFS, bw.records_of(ids, pos, mapq, 3), seed=4)
    with wt.BamReads(path, threads=1) as one, wt.BamReads(path, threads=8) as eight:
        _check(one, ids, pos, mapq, 3)
        assert np.array_equal(one.pos, eight.pos) and np.array_equal(one.mapq, eight.mapq)
        assert np.array_equal(one.offsets, eight.offsets)
        assert (one.mapped, one.unmapped, one.no_coordinate) == (eight.mapped, eight.unmapped, eight.no_coordinate)


def test_empty_references_and_no_records(tmp_path):
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, REFS, [])
    with wt.BamReads(path) as bam:
        assert len(bam.pos) == 0 and not bam.offsets.any() and bam.names[2] == "2"
    bw.write_bam(path, [], [(-1, -1, 0, 4)])
    with wt.BamReads(path) as bam:
        assert bam.names == [] and bam.no_coordinate == 1 and bam.unmapped == 1 and bam.mapped == 0


def _error(path):
    with pytest.raises(_lib.WisecondorHipError) as e:
        wt.BamReads(path, threads=2)
    assert len(str(e.value)) > 30
    return e.value.code, str(e.value)


def test_damaged_files_are_errors(tmp_path):
    ids, pos, mapq = _reads(5, n=1500)
    recs = bw.records_of(ids, pos, mapq, 2)
    data = bw.plain_bam(REFS, recs)
    good = bw.bgzf(data, list(range(5000, len(data), 5000)))
    path = str(tmp_path / "bad.bam")

    def put(blob):
        open(path, "wb").write(blob)
        return _error(path)

    assert _error(str(tmp_path / "missing.bam"))[0] == _lib.E_IO
    code, text = put(b"not a bam file at all, just some text that is long enough")
    assert code == _lib.E_FORMAT and "magic" in text
    code, text = put(bw.bgzf(b"SAM\x01" + data[4:]))
    assert code == _lib.E_FORMAT and "magic" in text
    assert put(b"")[0] == _lib.E_FORMAT
    # truncated: inside a block, inside a block header, and at a block boundary inside a record
    first = struct.unpack("<H", good[16:18])[0] + 1
    assert put(good[:first + 100])[0] == _lib.E_FORMAT
    assert put(good[:first + 7])[0] == _lib.E_FORMAT
    code, text = put(good[:first])
    assert code == _lib.E_FORMAT and ("overruns" in text or "header" in text)
    # damaged deflate data / CRC / size fields
    for at in (first + 30, first + 18 + 5):
        blob = bytearray(good)
        blob[at] ^= 0x55
        assert put(bytes(blob))[0] == _lib.E_FORMAT
    second = first + struct.unpack("<H", good[first + 16:first + 18])[0] + 1
    blob = bytearray(good)
    blob[second - 8] ^= 1                               # the CRC of block 2
    assert put(bytes(blob))[0] == _lib.E_FORMAT
    blob = bytearray(good)
    blob[first + 16:first + 18] = struct.pack("<H", 20)  # a block size smaller than its own header
    assert put(bytes(blob))[0] == _lib.E_FORMAT
    # a record whose block_size overruns the data, and one whose fields overrun its block_size
    head = len(bw.plain_bam(REFS, []))
    broken = bytearray(data)
    broken[head:head + 4] = struct.pack("<i", len(data))
    code, text = put(bw.bgzf(bytes(broken)))
    assert code == _lib.E_FORMAT and "overruns" in text
    broken = bytearray(data)
    broken[head + 4 + 16:head + 4 + 20] = struct.pack("<i", 1 << 20)         # l_seq
    code, text = put(bw.bgzf(bytes(broken)))
    assert code == _lib.E_FORMAT and "overrun" in text
    broken = bytearray(data)
    broken[head:head + 4] = struct.pack("<i", 8)
    assert put(bw.bgzf(bytes(broken)))[0] == _lib.E_FORMAT
    broken = bytearray(data)
    broken[head + 4:head + 8] = struct.pack("<i", 99)                           # refID beyond the header
    assert put(bw.bgzf(bytes(broken)))[0] == _lib.E_FORMAT


def test_unsorted_files_are_argument_errors(tmp_path):
    path = str(tmp_path / "bad.bam")
    bw.write_bam(path, REFS, [(0, 10, 60, 0), (0, 9, 60, 0)])
    code, text = _error(path)
    assert code == _lib.E_ARG and "coordinate-sorted" in text
    bw.write_bam(path, REFS, [(0, 10, 60, 0), (2, 5, 60, 0), (0, 20, 60, 0)])
    code, text = _error(path)
    assert code == _lib.E_ARG and "coordinate-sorted" in text
    bw.write_bam(path, REFS, [(0, 10, 60, 0), (-1, -1, 0, 4), (0, 10, 60, 0), (2, 5, 60, 0)])   # unplaced in between is fine
    with wt.BamReads(path) as bam:
        assert list(bam.pos) == [10, 10, 5] and list(bam.offsets) == [0, 2, 2, 3, 3, 3, 3]
