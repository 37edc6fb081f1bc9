"""k_bg_inflate (csrc/bamgpu.hip) on deflate streams zlib never writes, and its refusals against zlib's: the cases and
the mutant corpus of tests/inflate_cases.py (test_inflate_cases_cpu.py holds them to what they claim, on the CPU).  Byte
equality with zlib for what zlib takes, WC_E_FORMAT with the inflate status for what zlib refuses; then a BAM file whose
BGZF members the test's writer wrote, through the three readers and convert."""
import zlib

import numpy as np
import pytest

import bam_writer as bw
import deflate_writer as dw
import inflate_cases as ic
import test_bamgpu_gpu as old
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

pytestmark = pytest.mark.gpu

LEGAL = ic.legal_cases()
REFUSALS = ic.refusal_cases()


def _want(case):
    return b"".join(zlib.decompress(raw, -15) for raw, _ in case.parts)


def _refused(blob, cap, what):
    """The inflate status of the first member, not its CRC and not the directory: the deflate data itself was refused."""
    try:
        old._gpu_inflate(blob, cap)
    except _lib.WisecondorHipError as e:
        assert e.code == _lib.E_FORMAT and "block 0 (inflate failed)" in str(e), (what, str(e))
        return
    pytest.fail("inflated without complaint: %s" % (what,))


@pytest.mark.parametrize("case", LEGAL, ids=[c.name for c in LEGAL])
def test_legal_streams_inflate_to_zlibs_bytes(case):
    want = _want(case)
    assert old._gpu_inflate(b"".join(ic.members(case.parts)), len(want)) == want
    for m, (raw, _) in zip(ic.members(case.parts), case.parts):         # and every member alone, at the front of the buffer
        assert old._gpu_inflate(m, 65536) == zlib.decompress(raw, -15)


@pytest.mark.parametrize("r", REFUSALS, ids=[r.name for r in REFUSALS])
def test_refusals_are_format_errors_of_the_inflate_stage(r):
    with pytest.raises(zlib.error):
        zlib.decompress(r.raw, -15)
    _refused(dw.member(r.piece, r.raw), 65536, r.name)


def test_a_legal_stream_after_each_refusal():
    case = LEGAL[0]
    want, blob = _want(case), b"".join(ic.members(case.parts))
    picked = [r for r in REFUSALS if not r.name.startswith("a dynamic block cut")] + REFUSALS[-3:]
    for r in picked[::4]:
        _refused(dw.member(r.piece, r.raw), 65536, r.name)
        assert old._gpu_inflate(blob, len(want)) == want, r.name
    # a refused member between legal ones: the call names it
    a, b = ic.members(LEGAL[4].parts)[0], dw.member(REFUSALS[0].piece, REFUSALS[0].raw)
    with pytest.raises(_lib.WisecondorHipError) as e:
        old._gpu_inflate(a + b + a, 3 * 65536)
    assert e.value.code == _lib.E_FORMAT and "block 1 (inflate failed)" in str(e.value)


def test_all_legal_members_in_one_launch():
    """Every member of every legal case four times over, in a seeded order: a few hundred waves of mixed block types side
    by side, each member at other offsets of the buffer than when it ran alone."""
    parts = [part for case in LEGAL for part in case.parts] * 4
    parts = [parts[i] for i in np.random.RandomState(3).permutation(len(parts))]
    blob = b"".join(ic.members(parts))
    want = b"".join(zlib.decompress(raw, -15) for raw, _ in parts)
    assert len(parts) >= 200 and len({a for a in ic.data_alignments(parts)}) == 4
    assert old._gpu_inflate(blob, len(want) + 3) == want


def test_accepted_mutants_inflate_to_zlibs_bytes():
    accepted = ic.corpus().accepted
    assert len(accepted) > 1000
    blob = b"".join(dw.member(out, raw) for raw, out in accepted)
    want = b"".join(out for _, out in accepted)
    got = old._gpu_inflate(blob, len(want))
    if got != want:                                     # name the first mutant that differs
        at = 0
        for i, (raw, out) in enumerate(accepted):
            assert got[at:at + len(out)] == out, (i, raw[:ic.FLIP_BYTES].hex())
            at += len(out)
    assert got == want


def test_refused_mutants_are_format_errors_of_the_inflate_stage():
    refused = ic.corpus().refused
    assert 900 <= len(refused) <= 1600
    for i, (raw, message, piece) in enumerate(refused):
        _refused(dw.member(piece, raw), len(piece), (i, message, raw[:ic.FLIP_BYTES].hex()))
    # and the context is as it was
    assert old._gpu_inflate(b"".join(ic.members(LEGAL[1].parts)), 65536) == _want(LEGAL[1])


# ------------------------------------------------------------------------------------------------ a BAM by the writer
def _records():
    rng = np.random.RandomState(21)
    ids, pos, mapq = [], [], []
    for r, (_, length) in enumerate(old.CHROMS):
        k = 250
        ids.append(r)
        pos.append(np.sort(rng.randint(0, length, k)))
        mapq.append(rng.choice([0, 1, 19, 20, 37, 60], k))
    return bw.records_of(ids, pos, mapq, unplaced=3)


def test_bam_written_by_the_writer_through_every_reader_and_convert(tmp_path):
    data = bw.plain_bam(old.CHROMS, _records())
    ours, zlibs = str(tmp_path / "writer.bam"), str(tmp_path / "zlib.bam")
    blob = ic.bgzf_by_writer(data, 22, bw.EOF_BLOCK)
    assert b"".join(old._host_inflate(blob)) == data
    open(ours, "wb").write(blob)
    open(zlibs, "wb").write(bw.bgzf(data, list(range(9000, len(data), 9000))))
    arrays, offsets = old._same_as_host(ours)           # BamReadsDevice against BamReads, every array
    assert len(arrays[0]) == 24 * 250
    for chunk in (1, 30000, 1 << 30):
        with wt.BamReadsStream(ours, chunk=chunk) as dev:
            got = dev.to_numpy()
            assert np.array_equal(dev.offsets, offsets) and dev.n_reads == len(arrays[0])
            for g, w in zip(got, arrays):
                assert g.dtype == w.dtype and np.array_equal(g, w)
            assert chunk != 1 or dev.stream_info["chunks"] >= 20
    with wt.BamReadsDevice(zlibs) as dev:
        for g, w in zip(dev.to_numpy(), arrays):
            assert np.array_equal(g, w)
    want, want_q = wt.convertBam(zlibs, binsize=100000)
    got, got_q = wt.convertBam(ours, binsize=100000)
    with wt.openBamReads(ours) as dev:
        assert isinstance(dev, wt.BamReadsDevice)
    assert got_q == want_q and want_q["post_retro"] > 1000
    assert set(got) == set(want)
    for key in want:
        assert (got[key] is None) == (want[key] is None)
        if want[key] is not None:
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
