"""The deflate streams of tests/inflate_cases.py without a GPU: the writer against zlib (every legal case inflates to
model(tokens), every refusal raises zlib.error with the message its name stands for), the host reader's verdict on the same
members, a scanner that holds each case to what its name claims, the same scanner over the inputs of
test_bamgpu_gpu.py::test_inflate_matches_zlib_byte_for_byte, and the conditions on the mutant corpus."""
import os
import re
import struct
import zlib
from collections import Counter

import numpy as np
import pytest

import bam_writer as bw
import deflate_writer as dw
import inflate_cases as ic
import test_bamgpu_gpu as old
from wisecondor_amd import _lib
from wisecondor_amd import wisetools as wt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGAL = {c.name: c for c in ic.legal_cases()}


def _scanned(case):
    return [ic.scan(raw) for raw, _ in case.parts]


def _blocks(case):
    return [b for blocks, _, _ in _scanned(case) for b in blocks]


def test_table_widths_are_the_kernels():
    text = open(os.path.join(ROOT, "wisecondor_amd", "csrc", "bamgpu.hip")).read()
    m = re.search(r"const int BG_LIT_BITS = (\d+), BG_DIST_BITS = (\d+),", text)
    assert (int(m.group(1)), int(m.group(2))) == (ic.LIT_BITS, ic.DIST_BITS)


def test_writer_primitives():
    assert [dw.length_token(l) for l in (3, 10, 11, 12, 257, 258)] == [(257, 0), (264, 0), (265, 0), (265, 1), (284, 30), (285, 0)]
    assert [dw.distance_token(d) for d in (1, 4, 5, 6, 24577, 32768)] == [(0, 0), (3, 0), (4, 0), (4, 1), (29, 0), (29, 8191)]
    assert dw.canonical([3, 3, 3, 3, 3, 2, 4, 4]) == [(2, 3), (3, 3), (4, 3), (5, 3), (6, 3), (0, 2), (14, 4), (15, 4)]    # RFC 1951
    for n, top in ((16, 15), (286, 15), (286, 10), (30, 9), (19, 7)):
        for deep in (False, True):
            lens = dw.complete_lens(n, top, deep)
            assert len(lens) == n and max(lens) == top and dw.kraft(lens) == 32768
    assert dw.complete_lens(16, 15) == ic.CHAIN
    lens = [0] * 140 + [5] * 9 + [0, 0, 7, 7, 7] + [0] * 10
    assert dw.expand(dw.run_length(lens)) == lens and {s for s, _ in dw.run_length(lens)} == {18, 17, 16, 5, 7, 0}
    s = dw.BitSink()
    s.put(0b101, 3)
    s.code(0b110, 3)                                    # a code goes in first bit first: 1, 1, 0 behind the field's 1, 0, 1
    assert s.done() == bytes([0b00011101])
    assert dw.member(b"piece", b"\x03\x00") == old._block(b"piece", b"\x03\x00")    # the BGZF wrapper, restated
    data = old._text(5000, 9)
    assert dw.model(dw.tokens_of(data[1000:], data[:1000]), data[:1000]) == data[1000:]


def test_legal_cases_inflate_under_zlib_to_the_model():
    assert len(LEGAL) == len(ic.legal_cases()) >= 26
    for case in ic.legal_cases():
        for raw, piece in case.parts:                   # piece is model(tokens) behind the stored bytes
            assert zlib.decompress(raw, -15) == piece, case.name
            assert ic.zlib_verdict(raw) == (piece, None)
            assert len(piece) <= 65536 and len(raw) + 26 <= 65536
    # the second way to write 258: symbol 284 with all 5 extra bits set.  zlib 1.2.11 takes it
    d = dw.Deflate()
    d.fixed(1, [7, dw.Match(284, 31, 0, 0)])
    assert zlib.decompress(d.raw(), -15) == b"\x07" * 259


def test_refusal_cases_are_refused_by_zlib():
    names = [r.name for r in ic.refusal_cases()]
    assert len(set(names)) == len(names) >= 40
    for r in ic.refusal_cases():
        with pytest.raises(zlib.error) as e:
            zlib.decompress(r.raw, -15)
        if r.message is None:                           # the data ends early: zlib's one-shot call reports that as an error too
            assert "incomplete or truncated" in str(e.value), r.name
            assert ic.zlib_verdict(r.raw) == (None, None)
        else:
            assert r.message in str(e.value), (r.name, str(e.value))
    for m in ic.HEADER_AND_DISTANCE_MESSAGES:           # each of zlib's texts has a case of its own
        assert any(r.message and r.message in m for r in ic.refusal_cases()), m


# ------------------------------------------------------------------------------------------------ the host reader
REFS = [("chr1", 50000)]


def _as_bam(member_list, n):
    """A BAM file whose one record carries `n` tag bytes: everything before them in a member of zlib's, then `member_list`
    (which inflate to the tag bytes), then the EOF block."""
    rec = bw.record(0, 1, 30, l_seq=0, tags=bytes(n))
    front = bw.plain_bam(REFS, []) + rec[:len(rec) - n]
    return bw.bgzf_block(front) + b"".join(member_list) + bw.EOF_BLOCK


def test_host_reader_agrees_with_zlib_on_every_case(tmp_path):
    path = str(tmp_path / "case.bam")
    for case in ic.legal_cases():
        open(path, "wb").write(_as_bam(ic.members(case.parts), sum(len(p) for _, p in case.parts)))
        with wt.BamReads(path) as host:
            assert list(host.pos) == [1] and host.mapped == 1, case.name
    for r in ic.refusal_cases():
        open(path, "wb").write(_as_bam([dw.member(r.piece, r.raw)], len(r.piece)))
        with pytest.raises(_lib.WisecondorHipError) as e:
            wt.BamReads(path)
        assert e.value.code == _lib.E_FORMAT and "block 1 (inflate or CRC failed)" in str(e.value), (r.name, str(e.value))


# ------------------------------------------------------------------------------------------------ what the cases reach
def test_scanner_inflates_every_legal_case_like_zlib():
    for case in ic.legal_cases():
        for (blocks, out, used), (raw, piece) in zip(_scanned(case), case.parts):
            assert out == piece and used <= 8 * len(raw) and blocks[-1]["last"], case.name


def test_deep_trees_reach_fifteen_bits_on_both_codes():
    case = LEGAL["deep trees"]
    for blocks, _, _ in _scanned(case):
        for b in blocks:
            if b["type"] == 2:                          # every length 1..15 is in both sets
                assert set(b["lit_lens"]) == set(b["dist_lens"]) == set(range(16))
    r = ic.reach(_blocks(case))
    print("deep trees:", r)
    assert (r["lit_max"], r["dist_max"], r["lit_used"], r["dist_used"]) == (15, 15, 15, 15)
    assert r["lit_slow"] >= 30000 and r["dist_slow"] >= 6000
    by_len = sum((b["lit_by_len"] for b in _blocks(case) if b["type"]), Counter())
    assert by_len[15] >= 20000 and by_len[14] >= 50
    first = _blocks(case)[0]
    for dsym in (28, 29):                               # 5 extra bits of the length, then 15 + 13 bits of the distance
        assert first["matches"][(284, 31, dsym, 8191)] and first["dist_lens"][dsym] == 15 and dw.DIST_EXTRA[dsym] == 13
    assert dw.LEN_EXTRA[284 - 257] == 5 and first["lit_lens"][284] == 14


def test_table_edge_cases_sit_on_the_table_widths():
    seen = set()
    for case in ic.legal_cases():
        m = re.match(r"table edge: literal/length (\d+) bits, distance (\d+) bits", case.name)
        if not m:
            continue
        lit, dist = int(m.group(1)), int(m.group(2))
        r = ic.reach(_blocks(case))
        print(case.name, r)
        assert (r["lit_max"], r["dist_max"], r["lit_used"], r["dist_used"]) == (lit, dist, lit, dist)
        assert (r["lit_slow"] > 100) == (lit > ic.LIT_BITS) and (r["lit_slow"] == 0) == (lit == ic.LIT_BITS)
        assert (r["dist_slow"] > 20) == (dist > ic.DIST_BITS) and (r["dist_slow"] == 0) == (dist == ic.DIST_BITS)
        b = _blocks(case)[-1]
        assert b["lit_by_len"][lit] > 100 and b["dist_by_len"][dist] > 20 and min(b["lit_by_len"]) <= 2
        seen.add((lit, dist))
    assert seen == {(10, 9), (11, 10), (10, 10), (11, 9)} and (ic.LIT_BITS, ic.DIST_BITS) == (10, 9)


@pytest.mark.parametrize("name", ["every symbol, the fixed code", "every symbol, a dynamic 15-bit code"])
def test_every_symbol_pair_with_both_ends_of_its_extra_bits(name):
    matches = sum((b["matches"] for b in _blocks(LEGAL[name]) if b["type"]), Counter())
    # 3 480 matches; a symbol without extra bits has one value for both ends, so 2 744 of them differ
    assert set(matches) == set(ic.every_pair()) and sum(matches.values()) == 3480 == 29 * 30 * 4 and len(matches) == 2744
    assert {(k[0], k[2]) for k in matches} == {(l, d) for l in range(257, 286) for d in range(30)}
    assert matches[(285, 0, 29, 8191)] and matches[(284, 31, 29, 8191)] and matches[(257, 0, 0, 0)]
    for b in _blocks(LEGAL[name]):
        assert b["type"] == 0 and b["stored"] == 32768 or b["out_start"] == 32768      # distance 32 768 is legal everywhere
    if "dynamic" in name:
        b = _blocks(LEGAL[name])[1]
        assert all(b["lit_lens"]) and all(b["dist_lens"]) and b["hlit"] == 286 and b["hdist"] == 30 and b["lit_max"] == b["dist_max"] == 15


def test_overlapping_copies_around_the_wave_width():
    matches = sum((b["matches"] for b in _blocks(LEGAL["overlapping copies"])), Counter())
    got = {(dw.LEN_BASE[k[0] - 257] + k[1], dw.DIST_BASE[k[2]] + k[3]) for k in matches}
    assert got == set(ic.overlap_pairs())
    assert {(l, d) for d in (1, 2, 3, 63, 64, 65) for l in (3, 64, 65, 258)} <= got
    assert {(l, l + k) for l in (3, 64, 65, 258) for k in (-1, 0, 1)} <= got


def _dynamic(name, index=0):
    return [b for b in _blocks(LEGAL[name]) if b["type"] == 2][index]


def _crossing(b, symbol):
    """Code-length symbols `symbol` of block b whose run begins among the literal/length lengths and ends among the distances."""
    return [(p, s, e) for p, s, e in b["cl_syms"] if s == symbol and p < b["hlit"] < p + {16: 3, 17: 3, 18: 11}[s] + e]


def test_header_shapes_are_what_they_say():
    b = _dynamic("header: HLIT 257 and a lone distance length 0")
    assert (b["hlit"], b["hdist"], b["dist_lens"]) == (257, 1, [0]) and not b["matches"]
    b = _dynamic("header: HLIT 286")
    assert b["hlit"] == 286 and b["lit_lens"][285] and b["matches"][(285, 0, 0, 0)] and b["matches"][(284, 31, 0, 0)]
    b = _dynamic("header: HDIST 1 with length 1")
    assert (b["hdist"], b["dist_lens"]) == (1, [1]) and sum(b["matches"].values()) == 2
    b = _dynamic("header: HDIST 30")
    assert b["hdist"] == 30 and b["dist_lens"][29] and b["matches"][(257, 0, 29, 0)]
    b = _dynamic("header: HCLEN 5, the least that can name a length")
    assert b["hclen"] == 5 and b["hlit"] == 257
    b = _dynamic("header: HCLEN 19 and a code-length code of 7 bits")
    assert b["hclen"] == 19 and max(b["cl_lens"]) == 7 and all(b["cl_lens"])
    assert sum(1 for _, s, _ in b["cl_syms"] if b["cl_lens"][s] == 7) >= 4
    b = _dynamic("header: 18 with 138 zeros, 16 behind 17 and behind 18")
    syms = [(s, e) for _, s, e in b["cl_syms"]]
    assert (18, 127) in syms
    after = {(a[0], c[0]) for a, c in zip(syms[:-1], syms[1:])}
    assert (17, 16) in after and (18, 16) in after
    b = _dynamic("header: a 16 across the literal/distance boundary")
    assert _crossing(b, 16) and b["matches"][(259, 0, 7, 1)]
    b = _dynamic("header: an 18 across the literal/distance boundary")
    assert _crossing(b, 18) and b["matches"][(257, 0, 12, 0)] and b["matches"][(257, 0, 13, 31)]
    for name in ("header: empty blocks of a single 1-bit code", "header: a member that is one empty dynamic block"):
        for b in _blocks(LEGAL[name]):
            if b["type"] == 2:
                assert [(s, l) for s, l in enumerate(b["lit_lens"]) if l] == [(256, 1)] and sum(b["lit_by_len"].values()) == 1
    assert LEGAL["header: a member that is one empty dynamic block"].parts[0][1] == b""


def test_block_sequences_are_what_they_say():
    blocks = _blocks(LEGAL["sequence: stored, fixed, dynamic, empty stored, stored"])
    assert [b["type"] for b in blocks] == [0, 1, 2, 0, 0] and blocks[3]["stored"] == 0 and blocks[4]["stored"] > 0
    blocks = _blocks(LEGAL["sequence: stored blocks at every bit alignment"])
    assert sorted(b["start"] % 8 for b in blocks if b["type"] == 0) == list(range(8))
    blocks = _blocks(LEGAL["sequence: the largest stored block a member holds"])
    assert [b["stored"] for b in blocks] == [65505]
    raw = LEGAL["sequence: the largest stored block a member holds"].parts[0][0]
    assert len(dw.member(b"", raw)) == 65536           # one byte more and BSIZE would not hold the member's size
    (blocks, _, used), = _scanned(LEGAL["sequence: the last bit of the final block is the last bit of the input"])
    raw = LEGAL["sequence: the last bit of the final block is the last bit of the input"].parts[0][0]
    assert used == 8 * len(raw) and blocks[-1]["type"] == 1
    case = LEGAL["sequence: 1 to 4 unused bytes behind the final block"]
    unused = [len(raw) - (used + 7) // 8 for (_, _, used), (raw, _) in zip(_scanned(case), case.parts)]
    assert sorted(unused) == [1, 1, 2, 2, 3, 3, 4, 4]
    assert {b["type"] for b in _blocks(case)} == {0, 1}
    stored, dynamic, fixed = _blocks(LEGAL["sequence: matches that reach back into a stored and into a dynamic block"])
    assert (stored["type"], dynamic["type"], fixed["type"]) == (0, 2, 1)
    assert dynamic["sources"] and all(s < dynamic["out_start"] == 300 for s in dynamic["sources"])
    assert any(s < 300 for s in fixed["sources"]) and any(300 <= s < fixed["out_start"] for s in fixed["sources"])
    case = LEGAL["sequence: deflate data at every byte alignment of the file"]
    where = [a for a, (blocks, _, _) in zip(ic.data_alignments(case.parts), _scanned(case)) if blocks[0]["type"] == 2]
    assert set(where) == {0, 1, 2, 3}


# ------------------------------------------------------------------------------------------------ the old corpus
def test_what_the_zlib_written_corpus_reaches():
    """The inputs of test_bamgpu_gpu.py::test_inflate_matches_zlib_byte_for_byte (restated; its 1.2 MB file is more of
    "dynamic, level 6") under the scanner, zlib 1.2.11: literal/length codes up to 14 bits, distance codes up to 12, never
    15; 4 to 364 literal/length symbols per case beyond the 10-bit table in 6 of the 15 cases, 10 to 33 distance symbols
    beyond the 9-bit table in 3 of them; no repeat symbol across the literal/distance boundary; 418 of the 870 pairs of a
    length symbol with a distance symbol.  The new cases: 33 247 and 6 164 slow symbols in "deep trees" alone, all 870
    pairs with both ends of their extra bits."""
    rng = np.random.RandomState(7)
    text = old._text(60000)
    records = bw.plain_bam(old.REFS[:1], [(0, 3 * i, 30, 0) for i in range(800)])[:60000]
    runs = b"a" * 5000 + text[:20000] + b"\0" * 30000
    noise = rng.randint(0, 256, 65000).astype(np.uint8).tobytes()
    half = rng.randint(0, 256, 32768).astype(np.uint8).tobytes()
    every = bytes(range(256)) * 3
    _block, _deflate = old._block, old._deflate
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
        "distance 32768, length 258": [_block(half + half, old._far_stream(half))],
        "32768 random bytes twice, zlib's own blocks": [bw.bgzf(half + half, level=9)],
        "all byte values": [_block(every, _deflate(every))],
    }
    pairs, crossing, most = set(), 0, dict(lit_used=0, dist_used=0, lit_slow=0, dist_slow=0)
    for what, members in cases.items():
        blob, at, blocks = b"".join(members), 0, []
        while at < len(blob):
            size = struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
            got, out, _ = ic.scan(blob[at + 18:at + size - 8])
            assert out == zlib.decompress(blob[at + 18:at + size - 8], -15)
            blocks += got
            at += size
        r = ic.reach(blocks)
        print("%-45s %s" % (what, r))
        most = {k: max(v, r[k]) for k, v in most.items()}
        for b in blocks:
            if b["type"]:
                pairs |= {(k[0], k[2]) for k in b["matches"]}
            if b["type"] == 2:
                crossing += len(_crossing(b, 16)) + len(_crossing(b, 17)) + len(_crossing(b, 18))
    print("most:", most, "pairs:", len(pairs), "repeats across the boundary:", crossing)
    assert most["lit_used"] < 15 and most["dist_used"] < 15 and crossing == 0 and len(pairs) < 870
    if zlib.ZLIB_RUNTIME_VERSION == "1.2.11":
        assert most == dict(lit_used=14, dist_used=12, lit_slow=364, dist_slow=33) and len(pairs) == 418


# ------------------------------------------------------------------------------------------------ the mutants
def test_mutant_corpus_conditions():
    c = ic.corpus()
    n = len(c.accepted) + len(c.refused) + len(c.left_out)
    messages = Counter(m for _, m, _ in c.refused)
    print("mutants", n, "accepted", len(c.accepted), "refused", len(c.refused), "left out", len(c.left_out), dict(messages))
    assert n == 3 * 8 * ic.FLIP_BYTES
    assert len(c.accepted) >= 0.3 * n and len(c.refused) >= 0.3 * n and len(c.left_out) <= 0.05 * n
    assert set(messages) == set(ic.HEADER_AND_DISTANCE_MESSAGES)          # every one of them, and nothing else
    assert 900 <= len(c.refused) <= 1600                # a launch each on the GPU
    for raw, out in c.accepted[::37]:
        assert zlib.decompress(raw, -15) == out and len(out) <= 65536
        dw.member(out, raw)
    for raw, message, piece in c.refused[::37]:
        with pytest.raises(zlib.error):
            zlib.decompress(raw, -15)
        dw.member(piece, raw)
    assert c == ic.corpus.__wrapped__()                 # seeded: the same corpus every time


def test_bam_written_by_the_writer_is_the_data():
    data = bw.plain_bam(old.REFS, [(0, 7 * i, 30, 0) for i in range(1500)])
    blob = ic.bgzf_by_writer(data, 5, bw.EOF_BLOCK)
    assert b"".join(old._host_inflate(blob)) == data
    kinds, at, deep = Counter(), 0, 0
    while at < len(blob):
        size = struct.unpack("<H", blob[at + 16:at + 18])[0] + 1
        blocks, _, _ = ic.scan(blob[at + 18:at + size - 8])
        kinds.update(b["type"] for b in blocks)
        deep += ic.reach(blocks)["lit_slow"]
        at += size
    assert min(kinds[0], kinds[1], kinds[2]) >= 2 and deep > 3000
