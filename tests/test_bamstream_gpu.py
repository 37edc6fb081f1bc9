"""The streamed device BAM reader (wc_bam_stream_dev, BamReadsStream): bit for bit the host reader's result at chunk sizes
from one BGZF block to the whole file, chunk cuts inside a record (the carry), a record longer than several chunks, damaged
and unsorted files (the host reader's code, file-absolute offsets), convert end to end, and the memory bound: device working
bytes and pinned host bytes follow the chunk, not the file."""
import os
import re
import struct

import numpy as np
import pytest

import bam_writer as bw
import bam_writer_paired as bwp
import test_bamstream_cpu as cpu
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

pytestmark = pytest.mark.gpu

REFS = cpu.REFS
CHUNKS = [1, 4096, 70000, 1 << 30]


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


def _host(path):
    with wt.BamReads(path, threads=4) as host:
        return (host.names, host.lengths.copy(), host.offsets.copy(), (host.mapped, host.unmapped, host.no_coordinate),
                [a.copy() for a in (host.pos, host.mapq, host.flag, host.mate_pos)])


def _same_as_host(path, chunk, want=None):
    """The streamed reader's whole result equals the host reader's; returns (arrays, offsets, stream_info)."""
    names, lengths, offsets, counters, arrays = want or _host(path)
    with wt.BamReadsStream(path, chunk=chunk) as dev:
        got = dev.to_numpy()
        assert isinstance(dev, wt.BamReadsDevice)
        assert dev.names == names and np.array_equal(dev.lengths, lengths)
        assert np.array_equal(dev.offsets, offsets)
        assert (dev.mapped, dev.unmapped, dev.no_coordinate) == counters
        assert dev.n_reads == len(arrays[0])
        for g, w in zip(got, arrays):
            assert g.dtype == w.dtype and np.array_equal(g, w)
        info = dev.stream_info
        assert dev.device_bytes >= info["peak_device_working_bytes"] + 11 * dev.n_reads
        assert set(dev.stage_ms) == {"reader_wait", "device_wait", "call"} and dev.stage_ms["call"] > 0
        return got, dev.offsets.copy(), info


# ------------------------------------------------------------------------------------------------ 1. equality
@pytest.mark.parametrize("cuts", cpu.CUTS + ["regular_without_eof"])
def test_streamed_reader_equals_the_host_reader_at_every_chunk_size(tmp_path, cuts):
    assert _lib.load().wc_bam_chain_segment() == cpu.SEG
    ids, pos, mapq = _reads(1)
    data = bw.plain_bam(REFS, bw.records_of(ids, pos, mapq, unplaced=5))
    blob = bw.bgzf(data, eof=False) if cuts == "regular_without_eof" else cpu.blob_of(data, cuts)
    path = str(tmp_path / "a.bam")
    open(path, "wb").write(blob)
    want = _host(path)
    blocks = cpu.block_sizes(blob)
    for chunk in CHUNKS:
        (got_pos, got_mapq, _, _), offsets, info = _same_as_host(path, chunk, want)
        plan = cpu.chunking(blocks, chunk)
        assert info["chunks"] == len(plan)
        assert info["largest_chunk_compressed_bytes"] == max(p[1] for p in plan)
        assert info["largest_chunk_inflated_bytes"] == max(p[2] for p in plan)
        assert info["host_staging_bytes"] <= 2 * (min(chunk, len(blob)) + 65536 + cpu.BGZF_PAD) and info["pinned"] == 1
        for r in range(len(REFS)):
            a, b = int(offsets[r]), int(offsets[r + 1])
            if r in ids:
                assert np.array_equal(got_pos[a:b], pos[ids.index(r)]) and np.array_equal(got_mapq[a:b], mapq[ids.index(r)])
            else:
                assert a == b


def test_special_files(tmp_path):
    path = str(tmp_path / "a.bam")
    for chunk in (1, 1 << 30):
        bw.write_bam(path, REFS, [])                                                # no records
        arrays, offsets, _ = _same_as_host(path, chunk)
        assert len(arrays[0]) == 0 and not offsets.any()
        bw.write_bam(path, [], [(-1, -1, 0, 4)])                                    # no references
        with wt.BamReadsStream(path, chunk=chunk) as dev:
            assert dev.names == [] and (dev.mapped, dev.unmapped, dev.no_coordinate) == (0, 1, 1)
        _same_as_host(path, chunk)
        recs = [(0, 10, 60, 0), (-1, -1, 0, 4), (0, 10, 60, 0), (2, 5, 60, 0)]      # unplaced in between, references without reads
        bw.write_bam(path, REFS, recs, cuts=list(range(60, 2000, 60)))
        arrays, offsets, _ = _same_as_host(path, chunk)
        assert list(arrays[0]) == [10, 10, 5] and list(offsets) == [0, 2, 2, 3, 3, 3, 3]


# ------------------------------------------------------------------------------------------------ 2. cuts inside a record
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


def _record_starts(data, first):
    """[(inflated offset, refID)] of every record, by the block_size chain."""
    at, out = first, []
    while at < len(data):
        out.append((at, struct.unpack("<i", data[at + 4:at + 8])[0]))
        at += 4 + struct.unpack("<i", data[at:at + 4])[0]
    assert at == len(data)
    return out


def test_chunk_cuts_inside_records(tmp_path):
    starts = [3000 + 1500 * k for k in range(9)]
    data, recs = _padded_stream(starts)
    where = _record_starts(data, len(bw.plain_bam(REFS, [])))
    assert all(s in dict(where) for s in starts) and all(len(data) - s > 200 for s in starts)
    # a chunk ends 0 .. 36 bytes behind a record's start: the block_size word split 1/3, 2/2, 3/1, the fixed bytes split
    cuts = [s + d for s, d in zip(starts, (0, 1, 2, 3, 4, 35, 36))]
    cuts += [starts[7] + 2, starts[7] + 3]              # a carry of two bytes that survives a whole one-byte chunk
    cuts += [starts[8] + 1, starts[8] + 2, starts[8] + 3, starts[8] + 4]        # and one that grows byte by byte
    boundary = [a for (a, ref), (_, before) in zip(where[1:], where[:-1]) if ref == 2 and before == 0]
    assert len(boundary) == 1
    cuts.append(boundary[0])                            # the last record of one reference | the first of the next
    path = str(tmp_path / "cut.bam")
    open(path, "wb").write(bw.bgzf(data, cuts))         # the data ends with its last record: so does the last data chunk
    (pos, mapq, _, _), offsets, info = _same_as_host(path, 1)
    assert np.array_equal(pos, [r[1] for r in recs]) and np.array_equal(mapq, [r[2] for r in recs])
    assert offsets[1] == sum(1 for r in recs if r[0] == 0) and offsets[-1] == len(recs)
    assert info["chunks"] == len(set(cuts)) + 2         # the pieces and the EOF block
    assert info["largest_carry_bytes"] == 36            # every chunk ends at one of the cuts: the carries are their distances
    _same_as_host(path, 4096)
    # without the EOF block the file's last chunk ends with the last record
    open(path, "wb").write(bw.bgzf(data, cuts, eof=False))
    _same_as_host(path, 1)


# ------------------------------------------------------------------------------------------------ 3. a long record
def test_one_record_spans_four_chunks(tmp_path):
    head = bw.plain_bam(REFS, [])
    long_record = bw.record(0, 5, 30, l_seq=150000)
    assert len(long_record) == 225042
    tail = [bw.record(0, 10 + i, 20, l_seq=i % 50) for i in range(3000)]
    data = head + bw.record(0, 1, 1) + long_record + b"".join(tail)
    recs = [(0, 1, 1), (0, 5, 30)] + [(0, 10 + i, 20) for i in range(3000)]
    path = str(tmp_path / "long.bam")
    open(path, "wb").write(bw.bgzf(data, block=60000))
    (pos, mapq, _, _), offsets, info = _same_as_host(path, 1)
    assert np.array_equal(pos, [r[1] for r in recs]) and np.array_equal(mapq, [r[2] for r in recs])
    assert offsets[1] == len(recs)
    assert info["largest_chunk_inflated_bytes"] == 60000
    assert info["largest_carry_bytes"] >= 225042 - 60000      # more than a chunk: the buffer grew to hold the record


# ------------------------------------------------------------------------------------------------ 4. damaged files
def _codes(path, chunk):
    out = []
    for opener in (lambda p: wt.BamReads(p), lambda p: wt.BamReadsDevice(p), lambda p: wt.BamReadsStream(p, chunk=chunk)):
        with pytest.raises(_lib.WisecondorHipError) as e:
            opener(path)
        assert len(str(e.value)) > 30
        out.append((e.value.code, str(e.value)))
    return out


def _patched(blob, at, new):
    out = bytearray(blob)
    out[at:at + len(new)] = new
    return bytes(out)


def test_damaged_files_give_the_host_readers_code(tmp_path):
    ids, pos, mapq = _reads(5, n=1500)
    data = bw.plain_bam(REFS, bw.records_of(ids, pos, mapq, 2))
    cuts = list(range(5000, len(data), 5000))
    good = bw.bgzf(data, cuts)
    first = struct.unpack("<H", good[16:18])[0] + 1
    second = first + struct.unpack("<H", good[first + 16:first + 18])[0] + 1
    head = len(bw.plain_bam(REFS, []))
    where = [a for a, _ in _record_starts(data, head)]
    plan = cpu.chunking(cpu.block_sizes(good), 4096)
    assert len(plan) >= 8
    # inflated offsets at which the chunks of 4096 bytes begin: a record that starts in a middle chunk, one in the last
    begins = np.concatenate([[0], np.cumsum([p[2] for p in plan])])
    middle = [a for a in where if begins[len(plan) // 2] <= a < begins[len(plan) // 2 + 1]][1]
    last = where[-1]
    assert begins[-2] <= last and head < begins[1] <= middle
    path = str(tmp_path / "bad.bam")
    for chunk in (4096, 1):
        for what, blob in (("a flipped deflate byte", _patched(good, first + 30, bytes([good[first + 30] ^ 0x55]))),
                           ("a flipped CRC byte", _patched(good, second - 8, bytes([good[second - 8] ^ 1])))):
            open(path, "wb").write(blob)
            (host, _), (dev, dev_text), (stream, text) = _codes(path, chunk)
            assert host == dev == stream == _lib.E_FORMAT, what
            assert re.search(r"block (\d+)", text).group(1) == re.search(r"block (\d+)", dev_text).group(1) == "1", text
    for name, at in (("head", head), ("middle", middle), ("last", last)):
        cases = {
            "block_size overruns the data": _patched(data, at, struct.pack("<i", len(data))),
            "l_seq overruns block_size": _patched(data, at + 20, struct.pack("<i", 1 << 20)),
            "block_size 8": _patched(data, at, struct.pack("<i", 8)),
            "refID 99": _patched(data, at + 4, struct.pack("<i", 99)),
        }
        for what, bad in cases.items():
            open(path, "wb").write(bw.bgzf(bad, cuts))
            (host, _), (dev, dev_text), (stream, text) = _codes(path, 4096)
            assert host == dev == stream == _lib.E_FORMAT, (name, what)
            offset = re.search(r"inflated offset (\d+)", text).group(1)
            assert offset == re.search(r"inflated offset (\d+)", dev_text).group(1) == str(at), (name, what, text, dev_text)
            assert text == dev_text, (name, what)
    # truncated inside a record: the leftover behind the last chunk is an error, not a carry that is dropped
    for chunk in (1, 4096, 1 << 30):
        open(path, "wb").write(bw.bgzf(data[:len(data) - 17], cuts))
        (host, _), (dev, dev_text), (stream, text) = _codes(path, chunk)
        assert host == dev == stream == _lib.E_FORMAT and "truncated" in text and text == dev_text
        open(path, "wb").write(bw.bgzf(data[:len(data) - 17], cuts, eof=False))
        assert [c for c, _ in _codes(path, chunk)] == [_lib.E_FORMAT] * 3


# ------------------------------------------------------------------------------------------------ 5. unsorted files
def test_unsorted_files_are_argument_errors(tmp_path):
    path = str(tmp_path / "bad.bam")
    head = len(bw.plain_bam(REFS, []))
    rising = [(0, 10 + i, 60, 0) for i in range(40)]
    by_position = rising + [(0, 12, 60, 0)] + [(0, 100 + i, 60, 0) for i in range(40)]
    by_reference = rising + [(2, 5 + i, 60, 0) for i in range(30)] + [(0, 200, 60, 0)] + [(2, 300 + i, 60, 0) for i in range(10)]
    for recs, offender in ((by_position, 40), (by_reference, 70)):
        data = bw.plain_bam(REFS, recs)
        at = _record_starts(data, head)[offender][0]
        for cuts, chunk in (([at], 1), ([at - 3, at + 2], 1), ([at], 1 << 30), ([at - 100], 4096)):
            open(path, "wb").write(bw.bgzf(data, cuts))
            (host, _), (dev, dev_text), (stream, text) = _codes(path, chunk)
            assert host == dev == stream == _lib.E_ARG and "coordinate-sorted" in text
            assert text == dev_text, (text, dev_text)   # the same pair, numbered in the file


# ------------------------------------------------------------------------------------------------ 6. convert
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
    with wt.BamReads(path) as host, wt.BamReadsStream(path, chunk=4096) as dev:
        assert dev.stream_info["chunks"] > 24           # more chunks than chromosomes: towers and duplicates straddle them
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


def test_convert_from_the_streamed_reader_equals_the_host_reader(tmp_path):
    path = str(tmp_path / "s.bam")
    _sample_file(path, 1)
    _same_conversion(path)
    _, q = _same_conversion(path, mapq=20)
    assert q["filter_mapq"] > 1000
    _sample_file(path, 3, paired=True)
    _, q = _same_conversion(path, demandPair=True)
    assert q["pair_fail"] > 1000
    _sample_file(path, 4, paired=True, scrambled=True)
    _same_conversion(path, demandPair=True, mapq=20)


def test_stream_through_the_cli_and_the_reader_choice(tmp_path, monkeypatch):
    from wisecondor_amd import wisecondor as cli
    paths = [str(tmp_path / ("s%d.bam" % i)) for i in range(2)]
    for i, path in enumerate(paths):
        _sample_file(path, 7 + i)
    plain, streamed = str(tmp_path / "plain.npz"), str(tmp_path / "streamed.npz")
    cli.main(["convert", paths[0], plain, "-binsize", "100000"])
    cli.main(["convert", paths[0], streamed, "-binsize", "100000", "-stream", "-chunk", "65536"])
    a, b = np.load(plain, allow_pickle=True), np.load(streamed, allow_pickle=True)

    def same(a, b):
        sa, sb = a["sample"].item(), b["sample"].item()
        assert set(sa) == set(sb)
        for key in sa:
            assert sa[key].dtype == sb[key].dtype and sa[key].tobytes() == sb[key].tobytes()
        assert a["quality"].item() == b["quality"].item()

    same(a, b)
    assert "stream" not in a["arguments"].item() and "chunk" not in a["arguments"].item()
    assert b["arguments"].item()["stream"] is True and b["arguments"].item()["chunk"] == 65536
    outdir = str(tmp_path / "batch")
    cli.main(["convertbatch"] + paths + [outdir, "-binsize", "100000", "-stream"])
    c = np.load(os.path.join(outdir, "s0.npz"), allow_pickle=True)
    same(b, c)
    assert c["arguments"].item()["stream"] is True and "chunk" not in c["arguments"].item()
    assert c["arguments"].item()["infile"] == paths[0]
    single = str(tmp_path / "s1_single.npz")
    cli.main(["convert", paths[1], single, "-binsize", "100000", "-stream"])
    same(np.load(single, allow_pickle=True), np.load(os.path.join(outdir, "s1.npz"), allow_pickle=True))
    # the reader choice: the default is what it was
    assert wt.CONVERT_READER == "device"
    with wt.openBamReads(paths[0]) as bam:
        assert type(bam) is wt.BamReadsDevice
    with wt.openBamReads(paths[0], stream=True, chunk=4096) as bam:
        assert type(bam) is wt.BamReadsStream and bam.stream_info["chunks"] > 24
    monkeypatch.setattr(wt, "CONVERT_READER", "stream")
    with wt.openBamReads(paths[0]) as bam:
        assert type(bam) is wt.BamReadsStream
    monkeypatch.setattr(wt, "BAM_STREAM_CHUNK", 4096)
    with wt.openBamReads(paths[0]) as bam:
        assert bam.stream_info["chunks"] > 24
    monkeypatch.setattr(wt, "CONVERT_READER", "host")
    with wt.openBamReads(paths[0]) as bam:
        assert type(bam) is wt.BamReads


# ------------------------------------------------------------------------------------------------ 7. bounded memory
def test_working_memory_follows_the_chunk_and_not_the_file(tmp_path):
    """Peak device working bytes (everything except the four arrays) <= 2 N(c, t + carry) + 64 KiB, N the whole-file
    reader's need without its per-record term (cpu.working_need) for the largest chunk's compressed bytes c, its inflated
    bytes t and the largest carry: a condition, not a measurement.  The factor 2 is the double buffering.  A file four
    times as long may exceed the shorter one's working bytes only by twice the difference of that N between the two
    files' largest chunks.  The reader keeps inflated bytes in whole chain segments, so N takes t + carry rounded up to a
    whole segment for both files; the carry does not move either figure into another segment (asserted)."""
    chunk = 262144
    seen = []
    for n in (12500, 50000):
        refs, recs = cpu.big_records(n)
        path = str(tmp_path / ("r%d.bam" % n))
        bw.write_bam(path, refs, recs)
        blob = open(path, "rb").read()
        plan = cpu.chunking(cpu.block_sizes(blob), chunk)
        want = _host(path)
        first, offsets, info = _same_as_host(path, chunk, want)
        assert len(first[0]) == 4 * n
        again, offsets2, info2 = _same_as_host(path, chunk, want)           # two opens: identical arrays
        assert all(np.array_equal(a, b) for a, b in zip(first, again)) and np.array_equal(offsets, offsets2)
        assert info2 == info
        figures = (max(p[1] for p in plan), max(p[2] for p in plan), max(p[0] for p in plan))
        assert info["chunks"] == len(plan) >= 2
        assert (info["largest_chunk_compressed_bytes"], info["largest_chunk_inflated_bytes"]) == figures[:2]
        carry = info["largest_carry_bytes"]
        assert 0 < carry < 1000                         # a record of this writer
        bound = cpu.working_bound(figures[0], figures[1], carry, figures[2], len(refs))
        print("records", 4 * n, "chunks", len(plan), "working bytes", info["peak_device_working_bytes"], "bound", bound)
        assert info["peak_device_working_bytes"] <= bound
        assert info["host_staging_bytes"] <= 2 * (chunk + 65536 + cpu.BGZF_PAD) and info["pinned"] == 1
        seen.append((info["peak_device_working_bytes"], figures, carry, len(refs)))
    (w_small, f_small, carry_small, n_ref), (w_big, f_big, carry_big, _) = seen

    def need(figures, carry):
        assert (figures[1] + carry + cpu.SEG - 1) // cpu.SEG == (figures[1] + cpu.SEG - 1) // cpu.SEG
        whole = (figures[1] + carry + cpu.SEG - 1) // cpu.SEG * cpu.SEG
        return cpu.working_need(figures[0], whole, figures[2], n_ref)

    allowed = 2 * (need(f_big, carry_big) - need(f_small, carry_small))
    print("working bytes differ by", w_big - w_small, "allowed", allowed)
    assert w_big - w_small <= allowed
