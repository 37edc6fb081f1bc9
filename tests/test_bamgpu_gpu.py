"""The device BAM reader (csrc/bamgpu.hip): the inflate kernel against zlib byte for byte, the reader against the test's
own writer and the host reader (BamReads), record starts at the segment and block boundaries, damaged files (the host
reader's error code, never a fault), the device budget, convert end to end, repeatability."""
import os
import struct
import zlib

import numpy as np
import pytest

import bam_writer as bw
import bam_writer_paired as bwp
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

pytestmark = pytest.mark.gpu

SWEEP = int(os.environ.get("WC_SWEEP", "1"))
REFS = [("chr1", 50000), ("chrM", 16571), ("2", 40000), ("GL000207.1", 4262), ("chrX", 30000), ("chrY", 9000)]


# ------------------------------------------------------------------------------------------------ inflate
def _block(piece, cdata):
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cdata) + 25) + cdata
            + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))


def _deflate(piece, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush is None:
        return c.compress(piece) + c.flush()
    out, step = b"", max(1, len(piece) // 5)
    for i in range(0, len(piece), step):
        out += c.compress(piece[i:i + step]) + c.flush(flush)
    return out + c.flush()                              # every flush ends its deflate block with an empty stored one


def _far_stream(half):
    """A stored block of 32 768 bytes, then fixed-Huffman matches of distance 32 768 (zlib's own deflate stops 262 bytes
    short of that distance): 126 of length 258, one of 257, one of 3."""
    assert len(half) == 32768
    out = bytearray(b"\x00" + struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + half)
    acc = [0, 0]

    def put(value, nbits):                              # least significant bit first
        acc[0] |= value << acc[1]
        acc[1] += nbits
        while acc[1] >= 8:
            out.append(acc[0] & 255)
            acc[0] >>= 8
            acc[1] -= 8

    def code(value, nbits):                             # a Huffman code: most significant bit first
        put(int(format(value, "0%db" % nbits)[::-1], 2), nbits)

    def distance():
        code(29, 5)
        put(32768 - 24577, 13)

    put(1, 1)
    put(1, 2)
    for _ in range(126):
        code(0b11000101, 8)                             # 285: length 258
        distance()
    code(0b11000100, 8)                                 # 284: 227 + 5 extra bits
    put(30, 5)
    distance()
    code(0b0000001, 7)                                  # 257: length 3
    distance()
    code(0, 7)                                          # end of block
    if acc[1]:
        put(0, 8 - acc[1])
    return bytes(out)


def _gpu_inflate(blob, cap):
    lib = _lib.load()
    src = np.frombuffer(blob, dtype=np.uint8).copy()
    out = np.full(cap + 1, 0xA5, dtype=np.uint8)
    n = np.zeros(1, dtype=np.int64)
    _lib.check(lib.wc_bgzf_inflate(_lib.context(0), _lib.ptr(src), len(blob), _lib.ptr(out), cap, _lib.ptr(n)))
    assert out[cap] == 0xA5
    return out[:int(n[0])].tobytes()


def _text(n, seed=0):
    rng = np.random.RandomState(seed)
    words = [b"chr", b"read", b"\x00\x00\x00", b"ACGT", b"\xff\xff", b"NM", b"quality", b"\x10\x20\x30"]
    out = b"".join(words[i] + bytes([j & 255]) for i, j in zip(rng.randint(0, len(words), n // 4), rng.randint(0, 9, n // 4)))
    return out[:n]


def test_inflate_matches_zlib_byte_for_byte():
    rng = np.random.RandomState(7)
    text = _text(60000)
    records = bw.plain_bam(REFS[:1], [(0, 3 * i, 30, 0) for i in range(800)])[:60000]
    runs = b"a" * 5000 + text[:20000] + b"\0" * 30000
    noise = rng.randint(0, 256, 65000).astype(np.uint8).tobytes()
    half = rng.randint(0, 256, 32768).astype(np.uint8).tobytes()
    every = bytes(range(256)) * 3
    cases = {
        "stored": [_block(text, _deflate(text, 0))],
        "fixed Huffman": [_block(text, _deflate(text, 6, zlib.Z_FIXED))],
        "dynamic, level 1": [_block(records, _deflate(records, 1))],
        "dynamic, level 6": [_block(records, _deflate(records, 6))],
        "dynamic, level 9": [_block(text, _deflate(text, 9))],
        "no matches": [_block(text, _deflate(text, 6, zlib.Z_HUFFMAN_ONLY))],
        "distance-1 copies": [_block(runs, _deflate(runs, 6, zlib.Z_RLE))],
        "full flushes and an empty stored block": [_block(records, _deflate(records, 6, flush=zlib.Z_FULL_FLUSH))],
        "sync flushes and an empty stored block": [_block(text, _deflate(text, 6, flush=zlib.Z_SYNC_FLUSH))],
        "the EOF block in the middle": [_block(text, _deflate(text)), bw.EOF_BLOCK, _block(records, _deflate(records)), bw.EOF_BLOCK],
        "one byte": [_block(b"x", _deflate(b"x"))],
        "incompressible": [_block(noise, _deflate(noise))],
        "distance 32768, length 258": [_block(half + half, _far_stream(half))],
        "32768 random bytes twice, zlib's own blocks": [bw.bgzf(half + half, level=9)],
        "all byte values": [_block(every, _deflate(every))],
    }
    for what, blocks in cases.items():
        blob = b"".join(blocks)
        want = b"".join(_host_inflate(blob))
        got = _gpu_inflate(blob, len(want) + 7)
        assert got == want, what
    assert zlib.decompress(_far_stream(half), -15) == half + half
    big = (records * 25)[:1200000]
    blob = bw.bgzf(big, list(range(7, len(big), 1013)))
    assert blob.count(b"\x1f\x8b\x08\x04") >= 1180
    assert _gpu_inflate(blob, len(big)) == big
    assert _gpu_inflate(b"", 0) == b""


def _with_dictionary(piece):
    """`piece` deflated against itself as a preset dictionary: its matches point before the start of the output."""
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_DEFAULT_STRATEGY, piece)
    cdata = c.compress(piece) + c.flush()
    with pytest.raises(zlib.error):
        zlib.decompress(cdata, -15)
    return cdata


def _host_inflate(blob):
    at = 0
    while at < len(blob):
        size = struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
        yield zlib.decompress(blob[at + 18:at + size - 8], -15)
        at += size


def test_inflate_refuses_damaged_blocks_and_small_buffers():
    text = _text(30000, 3)
    blob = bw.bgzf(text, [10000, 20000])
    lib = _lib.load()
    for at in (40, len(blob) - len(bw.EOF_BLOCK) - 7):      # deflate data of block 0; the CRC of the last data block
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(_lib.WisecondorHipError) as e:
            _gpu_inflate(bytes(bad), len(text))
        assert e.value.code == _lib.E_FORMAT
    with pytest.raises(_lib.WisecondorHipError) as e:
        _gpu_inflate(blob, len(text) - 1)
    assert e.value.code == _lib.E_ARG
    # streams that end early, overrun ISIZE, or point before the start of the block: statuses, not faults
    for cdata, piece in ((_deflate(text[:5000])[:-20], text[:5000]), (_deflate(text[:5000]), text[:4000]),
                         (_with_dictionary(b"hello world, hello world"), b"hello world, hello world"), (b"", b"")):
        with pytest.raises(_lib.WisecondorHipError) as e:
            _gpu_inflate(_block(piece, cdata), 6000)
        assert e.value.code == _lib.E_FORMAT
    assert lib.wc_bam_chain_segment() >= 4096


# ------------------------------------------------------------------------------------------------ reader
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


def _same_as_host(path, threads=4):
    """The device reader's whole result equals the host reader's; returns the device arrays."""
    with wt.BamReads(path, threads=threads) as host, wt.BamReadsDevice(path) as dev:
        arrays = dev.to_numpy()
        assert dev.names == host.names and np.array_equal(dev.lengths, host.lengths)
        assert np.array_equal(dev.offsets, host.offsets)
        assert (dev.mapped, dev.unmapped, dev.no_coordinate) == (host.mapped, host.unmapped, host.no_coordinate)
        for got, want in zip(arrays, (host.pos, host.mapq, host.flag, host.mate_pos)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        return arrays, dev.offsets.copy()


@pytest.mark.parametrize("cuts", ["regular", "random", "tiny", "one_block_per_byte_of_header"])
def test_reader_returns_what_was_written(tmp_path, cuts):
    ids, pos, mapq = _reads(1)
    recs = bw.records_of(ids, pos, mapq, unplaced=5)
    data = bw.plain_bam(REFS, recs)
    if cuts == "regular":
        blob = bw.bgzf(data)
    elif cuts == "random":
        blob = bw.bgzf(data, sorted(np.random.RandomState(3).randint(1, len(data), 400).tolist()))
    elif cuts == "tiny":
        blob = bw.bgzf(data, list(range(7, len(data), 1013)), eof=False)
    else:
        blob = bw.bgzf(data, list(range(1, 200)) + [len(data) - 3, len(data) - 1])
    path = str(tmp_path / "a.bam")
    open(path, "wb").write(blob)
    (got_pos, got_mapq, got_flag, got_mate), offsets = _same_as_host(path)
    for r in range(len(REFS)):
        a, b = int(offsets[r]), int(offsets[r + 1])
        if r in ids:
            assert np.array_equal(got_pos[a:b], pos[ids.index(r)]) and np.array_equal(got_mapq[a:b], mapq[ids.index(r)])
        else:
            assert a == b
    placed = [r for r in recs if r[0] >= 0]
    assert np.array_equal(got_flag, [r[3] for r in placed]) and np.all(got_mate == -1)


@pytest.mark.parametrize("seed", range(3 * SWEEP))
def test_seeded_random_cuts(tmp_path, seed):
    ids, pos, mapq = _reads(10 + seed, n=1500 + 400 * seed)
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, REFS, bw.records_of(ids, pos, mapq, seed), seed=seed)
    _same_as_host(path)


def test_two_hundred_thousand_records_and_repeatability(tmp_path):
    rng = np.random.RandomState(5)
    refs = [("chr%d" % (c + 1), 2000000) for c in range(4)]
    recs = []
    for c in range(4):
        p = np.sort(rng.randint(0, 2000000, 50000))
        recs += list(zip([c] * 50000, p.tolist(), rng.randint(0, 61, 50000).tolist(), [0] * 50000))
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, refs, recs)
    first, offsets = _same_as_host(path, threads=8)
    assert len(first[0]) == 200000
    with wt.BamReadsDevice(path) as again:
        assert all(np.array_equal(a, b) for a, b in zip(first, again.to_numpy())) and np.array_equal(offsets, again.offsets)


def test_special_files(tmp_path):
    path = str(tmp_path / "a.bam")
    bw.write_bam(path, REFS, [])                                                # no records
    arrays, offsets = _same_as_host(path)
    assert len(arrays[0]) == 0 and not offsets.any()
    bw.write_bam(path, [], [(-1, -1, 0, 4)])                                    # no references
    with wt.BamReadsDevice(path) as dev:
        assert dev.names == [] and (dev.mapped, dev.unmapped, dev.no_coordinate) == (0, 1, 1)
    _same_as_host(path)
    bw.write_bam(path, REFS, [(0, 10, 60, 0), (-1, -1, 0, 4), (0, 10, 60, 0), (2, 5, 60, 0)])   # unplaced in between
    arrays, offsets = _same_as_host(path)
    assert list(arrays[0]) == [10, 10, 5] and list(offsets) == [0, 2, 2, 3, 3, 3, 3]


# ------------------------------------------------------------------------------------ segment and block boundaries
def _padded_stream(starts_at, n_tail=40):
    """A BAM stream in which a record starts at each of the inflated offsets `starts_at` (ascending, far enough apart):
    the record before each of them carries a tag that pads it to the byte.  Returns (data, records as written)."""
    head = bw.plain_bam(REFS, [])
    out, recs, at, k = [head], [], len(head), 0

    def add(rec, ref, pos, mapq):
        nonlocal at
        out.append(rec)
        recs.append((ref, pos, mapq))
        at += len(rec)

    for target in starts_at:
        while target - at > 400:
            add(bw.record(0, k, k % 61, l_seq=k % 90, n_cigar=k % 3), 0, k, k % 61)
            k += 1
        gap = target - at
        assert gap >= 100
        base = len(bw.record(0, k, 7, l_seq=5))
        add(bw.record(0, k, 7, l_seq=5, tags=b"Z" * (gap - base)), 0, k, 7)
        assert at == target
        k += 1
    for _ in range(n_tail):
        add(bw.record(2, k, 9, l_seq=k % 40), 2, k, 9)
        k += 1
    return b"".join(out), recs


def _check_stream(tmp_path, data, recs, cuts=None):
    path = str(tmp_path / "seg.bam")
    open(path, "wb").write(bw.bgzf(data, cuts))
    (pos, mapq, _, _), offsets = _same_as_host(path)
    assert np.array_equal(pos, [r[1] for r in recs]) and np.array_equal(mapq, [r[2] for r in recs])
    assert offsets[1] == sum(1 for r in recs if r[0] == 0) and offsets[-1] == len(recs)


def test_record_starts_around_segment_boundaries(tmp_path):
    seg = _lib.load().wc_bam_chain_segment()
    starts = [s * seg - d for s, d in zip(range(1, 8), (0, 1, 2, 3, 4, 35, 36))]
    data, recs = _padded_stream(starts)
    assert len(data) > 7 * seg
    _check_stream(tmp_path, data, recs)
    # the same record starts with BGZF blocks cut on and around the segment boundaries
    _check_stream(tmp_path, data, recs, [s * seg + d for s in range(1, 8) for d in (-2, 0, 3)])


def test_last_record_ends_on_a_segment_boundary(tmp_path):
    seg = _lib.load().wc_bam_chain_segment()
    data, recs = _padded_stream([2 * seg], n_tail=0)
    assert len(data) == 2 * seg
    _check_stream(tmp_path, data, recs)


def test_one_record_spans_several_blocks_and_segments(tmp_path):
    seg = _lib.load().wc_bam_chain_segment()
    head = bw.plain_bam(REFS, [])
    long_record = bw.record(0, 5, 30, l_seq=150000)
    assert len(long_record) == 225042 and len(long_record) > 3 * seg
    tail = [bw.record(0, 10 + i, 20, l_seq=i % 50) for i in range(3000)]
    data = head + bw.record(0, 1, 1) + long_record + b"".join(tail)
    recs = [(0, 1, 1), (0, 5, 30)] + [(0, 10 + i, 20) for i in range(3000)]
    _check_stream(tmp_path, data, recs)


# ------------------------------------------------------------------------------------------------ damaged files
def _both_codes(path):
    codes = []
    for cls in (wt.BamReads, wt.BamReadsDevice):
        with pytest.raises(_lib.WisecondorHipError) as e:
            cls(path)
        assert len(str(e.value)) > 30
        codes.append((e.value.code, str(e.value)))
    return codes


def test_damaged_files_give_the_host_readers_code(tmp_path):
    ids, pos, mapq = _reads(5, n=1500)
    data = bw.plain_bam(REFS, bw.records_of(ids, pos, mapq, 2))
    good = bw.bgzf(data, list(range(5000, len(data), 5000)))
    first = struct.unpack("<H", good[16:18])[0] + 1
    second = first + struct.unpack("<H", good[first + 16:first + 18])[0] + 1
    head = len(bw.plain_bam(REFS, []))
    path = str(tmp_path / "bad.bam")

    def patched(blob, at, new):
        out = bytearray(blob)
        out[at:at + len(new)] = new
        return bytes(out)

    cases = {
        "a flipped deflate byte": patched(good, first + 30, bytes([good[first + 30] ^ 0x55])),
        "a flipped CRC byte": patched(good, second - 8, bytes([good[second - 8] ^ 1])),
        "block_size overruns the data": bw.bgzf(patched(data, head, struct.pack("<i", len(data)))),
        "l_seq overruns block_size": bw.bgzf(patched(data, head + 20, struct.pack("<i", 1 << 20))),
        "block_size 8": bw.bgzf(patched(data, head, struct.pack("<i", 8))),
        "refID 99": bw.bgzf(patched(data, head + 4, struct.pack("<i", 99))),
        "truncated inside a record": bw.bgzf(data[:len(data) - 17]),
    }
    for what, blob in cases.items():
        open(path, "wb").write(blob)
        (host, _), (dev, _) = _both_codes(path)
        assert host == dev == _lib.E_FORMAT, what


def test_unsorted_files_are_argument_errors(tmp_path):
    path = str(tmp_path / "bad.bam")
    for recs in ([(0, 10, 60, 0), (0, 9, 60, 0)], [(0, 10, 60, 0), (2, 5, 60, 0), (0, 20, 60, 0)]):
        bw.write_bam(path, REFS, recs)
        for code, text in _both_codes(path):
            assert code == _lib.E_ARG and "coordinate-sorted" in text


# ------------------------------------------------------------------------------------------------ budget, convert
CHROMS = [("chr%d" % c, 3000000) for c in range(1, 23)] + [("chrX", 2000000), ("chrY", 1000000)]


def _sample_file(path, seed, paired=False, scrambled=False):
    rng = np.random.RandomState(seed)
    refs = list(CHROMS)
    if scrambled:                                       # references the conversion skips, between those it picks
        refs = refs[:3] + [("GL000207.1", 50000)] + refs[3:10] + [("chrM", 16571)] + refs[10:]
    recs = []
    for r, (name, length) in enumerate(refs):
        k = 2500 if not name.startswith("GL") else 300
        p = np.sort(rng.randint(0, length, k))
        p[k // 2:k // 2 + 40] = p[k // 2] + np.arange(40)       # a tower for the RETRO filter
        p = np.sort(p)
        q = rng.choice([0, 1, 19, 20, 37, 60], k)
        if paired:
            f = rng.choice([0x1 | 0x2 | 0x40, 0x1 | 0x2 | 0x80, 0x1 | 0x40, 0x0], k)
            m = p + rng.choice([0, 150, 150, 300], k)
            recs += bwp.records_of([r], [p], [q], [f], [m])
        else:
            recs += bw.records_of([r], [p], [q])
    (bwp if paired else bw).write_bam(path, refs, recs + ([(-1, -1, 0, 5, -1)] * 3 if paired else [(-1, -1, 0, 4)] * 3), seed=seed)


def _same_conversion(path, **kw):
    with wt.BamReads(path) as host, wt.BamReadsDevice(path) as dev:
        want, want_q = wt.convertBamReads(host, binsize=100000, **kw)
        got, got_q = wt.convertBamReads(dev, binsize=100000, **kw)
    assert got_q == want_q
    assert set(got) == set(want)
    for key in want:
        assert (got[key] is None) == (want[key] is None), key
        if want[key] is not None:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert want_q["post_retro"] > 1000
    return want, want_q


def test_convert_from_the_device_reader_equals_the_host_reader(tmp_path):
    path = str(tmp_path / "s.bam")
    _sample_file(path, 1)
    _same_conversion(path)
    _, q = _same_conversion(path, mapq=20)
    assert q["filter_mapq"] > 1000
    _sample_file(path, 2, scrambled=True)               # the picked references are not contiguous: gathered on the device
    _same_conversion(path)
    _sample_file(path, 3, paired=True)
    _, q = _same_conversion(path, demandPair=True)
    assert q["pair_fail"] > 1000
    _sample_file(path, 4, paired=True, scrambled=True)
    _same_conversion(path, demandPair=True, mapq=20)


def test_one_byte_budget_is_a_limit_error_and_convert_takes_the_host_reader(tmp_path, monkeypatch):
    path = str(tmp_path / "s.bam")
    _sample_file(path, 6)
    with pytest.raises(_lib.WisecondorHipError) as e:
        wt.BamReadsDevice(path, budget=1)
    assert e.value.code == _lib.E_LIMIT and "budget 1" in str(e.value) and "needs" in str(e.value)
    with wt.BamReads(path) as host:
        want, want_q = wt.convertBamReads(host, binsize=100000)
    monkeypatch.setattr(wt, "CONVERT_READER", "device")
    monkeypatch.setattr(wt, "BAM_DEVICE_BUDGET", 1)
    assert isinstance(wt.openBamReads(path), wt.BamReads)
    got, got_q = wt.convertBam(path, binsize=100000)
    assert got_q == want_q and all(np.array_equal(got[k], want[k]) for k in want)
    monkeypatch.setattr(wt, "BAM_DEVICE_BUDGET", 0)
    with wt.openBamReads(path) as dev:
        assert isinstance(dev, wt.BamReadsDevice)
    got, got_q = wt.convertBam(path, binsize=100000)
    assert got_q == want_q and all(np.array_equal(got[k], want[k]) for k in want)
