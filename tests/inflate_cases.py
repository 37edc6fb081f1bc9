"""Named deflate streams for the inflate kernel (csrc/bamgpu.hip, k_bg_inflate), written by tests/deflate_writer.py: legal
streams that zlib's own deflate never produces (deep trees, code lengths at the kernel's table widths, every length and
distance symbol at both ends of its extra bits, overlapping copies, odd dynamic headers, block sequences), streams that
must be refused, and a seeded corpus of single-bit mutants of zlib streams that zlib itself sorts into accepted and
refused.  zlib's verdict (`zlib.decompress(raw, -15)`) is the definition of legal; no device is needed to build any of this.
`scan` is a plain inflate that reports what a stream makes a decoder do (test_inflate_cases_cpu.py holds every case to
what its name claims)."""
import functools
import zlib
from collections import Counter, namedtuple

import numpy as np

import deflate_writer as dw
from deflate_writer import Bits, Deflate, Dist, Match, Sym

LIT_BITS, DIST_BITS = 10, 9     # BG_LIT_BITS, BG_DIST_BITS: test_inflate_cases_cpu.py asserts that the kernel source says the same

# parts: [(raw deflate stream, the bytes it inflates to)], one BGZF member each
Legal = namedtuple("Legal", "name parts")
# piece: what a decoder without the rule would put out (ISIZE and CRC of the member are made of it, so only the rule
# stands between the stream and a clean status); message: part of zlib's text for it
Refusal = namedtuple("Refusal", "name raw piece message")


def _noise(n, seed):
    return np.random.RandomState(seed).randint(0, 256, n).astype(np.uint8).tobytes()


def _shuffled(values, seed):
    values = list(values)
    np.random.RandomState(seed).shuffle(values)
    return values


def members(parts):
    return [dw.member(piece, raw) for raw, piece in parts]


# ------------------------------------------------------------------------------------------------ 1. deep trees
CHAIN = list(range(1, 15)) + [15, 15]           # the one complete set with every length 1..15 present: 16 symbols
DEEP_LIT_SYMS = [256, 257, 258, ord("N"), 264, 265, 273, 277, 285, 0, 281, ord("T"), ord("G"), 284, ord("A"), ord("C")]
DEEP_DIST_SYMS = [5, 20, 15, 10, 4, 3, 2, 1, 0, 23, 24, 25, 26, 27, 28, 29]
DEEP_LIT = dw.spread(286, DEEP_LIT_SYMS, CHAIN)
DEEP_DIST = dw.spread(30, DEEP_DIST_SYMS, CHAIN)


def _deep_trees():
    rng = np.random.RandomState(11)
    # member 1: 33 000 literals on codes of 12 to 15 bits, then long matches: a length code with 5 extra bits, then a
    # 15-bit distance code with 13 extra bits
    tokens = [int(c) for c in rng.choice([ord(c) for c in "ACGT"], 33000, p=[0.4, 0.4, 0.1, 0.1])]
    tokens += [Match(284, 31, 28, 8191), Match(284, 31, 29, 8191)]    # 14 + 5 bits, then 15 + 13 bits
    op = len(tokens) - 2 + 2 * 258
    while True:
        lsym = int(rng.choice([281, 284]))
        m = Match(lsym, int(rng.randint(0, 32)), int(rng.choice([28, 29])), 0)
        length = dw.LEN_BASE[lsym - 257] + m.lextra
        if op + length > 65536:
            break
        room = min(op - dw.DIST_BASE[m.dsym], 8191)
        m = m._replace(dextra=int(rng.randint(0, room + 1)))
        tokens.append(m)
        op += length
    d = Deflate()
    d.dynamic(1, DEEP_LIT, DEEP_DIST, tokens)
    one = (d.raw(), dw.model(tokens))
    # member 2: a stored half, then 6 000 three-byte matches whose distance symbols all sit on the 14- and 15-bit codes
    half = _noise(32768, 12)
    tokens, op = [], 32768
    for i in range(6000):
        dsym = int(rng.choice([27, 28, 29]))
        tokens.append(Match(257, 0, dsym, int(rng.randint(0, min(op - dw.DIST_BASE[dsym], (1 << dw.DIST_EXTRA[dsym]) - 1) + 1))))
        op += 3
        if i % 50 == 0:
            tokens.append(int(rng.choice([ord("A"), ord("C"), ord("G"), ord("T"), 0, ord("N")])))
            op += 1
    d = Deflate()
    d.stored(0, half)
    d.dynamic(1, DEEP_LIT, DEEP_DIST, tokens)
    return Legal("deep trees", [one, (d.raw(), half + dw.model(tokens, half))])


# ------------------------------------------------------------------------------------------------ 2. table edges
def _edge_member(lit_max, dist_max, seed):
    lit = dw.spread(286, _shuffled(range(286), seed), dw.complete_lens(286, lit_max, deep=True))
    dist = dw.spread(30, _shuffled(range(30), seed + 1), dw.complete_lens(30, dist_max, deep=True))
    rng = np.random.RandomState(seed + 2)
    half = _noise(32768, seed + 3)
    tokens = _shuffled(list(range(256)) * 2, seed + 4)
    for k in range(3):                                  # every length symbol and every distance symbol, three times
        for lsym, dsym in zip(_shuffled(range(257, 286), seed + 5 + k), _shuffled(range(30), seed + 8 + k)[:29]):
            tokens.append(Match(lsym, int(rng.randint(0, 1 << dw.LEN_EXTRA[lsym - 257])), dsym, int(rng.randint(0, 1 << dw.DIST_EXTRA[dsym]))))
            tokens.append(int(rng.randint(0, 256)))
        tokens.append(Match(257 + k, 0, _shuffled(range(30), seed + 8 + k)[29], 0))
    d = Deflate()
    d.stored(0, half)
    d.dynamic(1, lit, dist, tokens)
    return d.raw(), half + dw.model(tokens, half)


def _table_edges():
    return [Legal("table edge: literal/length %d bits, distance %d bits" % (l, d), [_edge_member(l, d, 100 * l + d)])
            for l, d in ((LIT_BITS, DIST_BITS), (LIT_BITS + 1, DIST_BITS + 1), (LIT_BITS, DIST_BITS + 1), (LIT_BITS + 1, DIST_BITS))]


# ------------------------------------------------------------------------------------------------ 3. every symbol
def every_pair():
    """29 x 30 symbol pairs, each with the least and the greatest extra bits of both: 3 480 matches."""
    out = []
    for lsym in range(257, 286):
        for dsym in range(30):
            for le in (0, (1 << dw.LEN_EXTRA[lsym - 257]) - 1):
                for de in (0, (1 << dw.DIST_EXTRA[dsym]) - 1):
                    out.append(Match(lsym, le, dsym, de))
    assert len(out) == 3480
    return out


def _every_symbol(dynamic, seed):
    lit = dw.spread(286, _shuffled(range(286), seed), dw.complete_lens(286, 15))
    dist = dw.spread(30, _shuffled(range(30), seed + 1), dw.complete_lens(30, 15))
    todo = _shuffled(every_pair(), seed + 2)
    parts = []
    while todo:
        half = _noise(32768, seed + 3 + len(parts))
        tokens, op = [], 32768
        while todo:
            length = dw.LEN_BASE[todo[-1].lsym - 257] + todo[-1].lextra
            if op + length > 65536:
                break
            tokens.append(todo.pop())
            op += length
        d = Deflate()
        d.stored(0, half)
        if dynamic:
            d.dynamic(1, lit, dist, tokens)
        else:
            d.fixed(1, tokens)
        parts.append((d.raw(), half + dw.model(tokens, half)))
    return Legal("every symbol, %s code" % ("a dynamic 15-bit" if dynamic else "the fixed"), parts)


# ------------------------------------------------------------------------------------------------ 4. overlapping copies
OVERLAP_DISTANCES = (1, 2, 3, 63, 64, 65)
OVERLAP_LENGTHS = (3, 64, 65, 258)


def overlap_pairs():
    out = [(l, d) for d in OVERLAP_DISTANCES for l in OVERLAP_LENGTHS]
    out += [(l, d) for l in OVERLAP_LENGTHS for d in (l, l - 1, l + 1)]
    return out


def _overlaps():
    rng = np.random.RandomState(41)
    tokens = [int(b) for b in rng.randint(0, 256, 300)]
    for pair in overlap_pairs():
        tokens.append(pair)
        tokens += [int(b) for b in rng.randint(0, 256, 3)]
    d = Deflate()
    d.fixed(1, tokens)
    return Legal("overlapping copies", [(d.raw(), dw.model(tokens))])


# ------------------------------------------------------------------------------------------------ 5. header shapes
def _one(name, build):
    d = Deflate()
    piece = build(d)
    return Legal(name, [(d.raw(), piece)])


def _small_lit(n_lit, extra=()):
    """'a', 'b', 'c' and 256 on 2-bit codes, or with `extra` symbols: a, b on 2 bits and the rest as even as it goes."""
    if not extra:
        return dw.spread(n_lit, [97, 98, 99, 256], [2, 2, 2, 2])
    rest = [99, 256] + list(extra)
    flat = [l + 1 for l in dw.flat_code(range(len(rest)), len(rest))]
    return dw.spread(n_lit, [97, 98] + rest, [2, 2] + flat)


def _header_shapes():
    out = []
    abc = [97, 98, 99, 97, 97, 98] * 5

    def hlit_min(d):                                    # HLIT 257, HDIST 1 with that one length 0: no distance code
        d.dynamic(1, _small_lit(257), [0], abc)
        return dw.model(abc)
    out.append(_one("header: HLIT 257 and a lone distance length 0", hlit_min))

    def hlit_max(d):
        tokens = abc + [(258, 1), Match(284, 31, 0, 0), 99]
        d.dynamic(1, _small_lit(286, [284, 285]), [1, 1], tokens)
        return dw.model(tokens)
    out.append(_one("header: HLIT 286", hlit_max))

    def huffman_only(d):                                # one distance code of one bit: an incomplete set zlib takes
        tokens = abc + [(3, 1), 98, (10, 1)]
        d.dynamic(1, _small_lit(266, [257, 264]), [1], tokens)
        return dw.model(tokens)
    out.append(_one("header: HDIST 1 with length 1", huffman_only))

    def hdist_max(d):
        far = _noise(24600, 51)
        tokens = abc + [Match(257, 0, 29, 0), Match(257, 0, 29, 23), (3, 1)]
        d.stored(0, far)
        d.dynamic(1, _small_lit(258, [257]), dw.spread(30, [0, 29], [1, 1]), tokens)
        return far + dw.model(tokens, far)
    out.append(_one("header: HDIST 30", hdist_max))

    def hclen_min(d):                                   # 16 17 18 0 8: with four of them every length would be 0
        lit = [0] + [8] * 256
        tokens = list(range(1, 256)) + [255, 1]
        d.dynamic(1, lit, [0], tokens, header=dict(cl_lens=dw.spread(19, [8, 0, 18], [1, 2, 2]), hclen=5,
                                                   cl_syms=[(0, None)] + [(8, None)] * 256 + [(0, None)]))
        return dw.model(tokens)
    out.append(_one("header: HCLEN 5, the least that can name a length", hclen_min))

    def hclen_max(d):                                   # the code-length code on 7-bit codes, its last length in use
        tokens = [ord(c) for c in "ACGTNACCA"] + [0, (3, 1), (10, 2), (4, 3), Match(281, 9, 1, 0)]
        cl = dw.spread(19, [18, 17, 16] + list(range(1, 14)) + [14, 0, 15], dw.complete_lens(19, 7))
        assert cl[0] == cl[15] == 7
        d.dynamic(1, DEEP_LIT, DEEP_DIST, tokens, header=dict(cl_lens=cl, hclen=19))
        return dw.model(tokens)
    out.append(_one("header: HCLEN 19 and a code-length code of 7 bits", hclen_max))

    def long_zero_run(d):                               # 18 with 138 zeros, and a 16 behind a 17 and behind an 18
        lit = dw.spread(286, [200, 201, 256, 280], [2, 2, 2, 2])
        syms = [(18, 127), (18, 62 - 11), (2, None), (2, None), (17, 0), (16, 0), (18, 42 - 11), (16, 3), (2, None),
                (18, 23 - 11), (2, None), (17, 2), (1, None), (1, None)]
        assert dw.expand(syms) == lit + [1, 1]
        tokens = [200, 201, 200, Match(280, 0, 1, 0), Match(280, 15, 0, 0)]
        d.dynamic(1, lit, [1, 1], tokens, header=dict(cl_syms=syms))
        return dw.model(tokens)
    out.append(_one("header: 18 with 138 zeros, 16 behind 17 and behind 18", long_zero_run))

    def sixteen_across(d):                              # lengths 3 3 3 3 | 3 x 8: the first 16 runs over the boundary
        lit = dw.spread(260, [97, 98, 256, 257, 258, 259], [2, 2, 3, 3, 3, 3])
        syms = [(18, 97 - 11), (2, None), (2, None), (18, 127), (18, 19 - 11), (3, None), (16, 3), (16, 2)]
        assert dw.expand(syms) == lit + [3] * 8
        tokens = [97, 98] * 10 + [Match(259, 0, 7, 1), Match(257, 0, 0, 0)]
        d.dynamic(1, lit, [3] * 8, tokens, header=dict(cl_syms=syms))
        return dw.model(tokens)
    out.append(_one("header: a 16 across the literal/distance boundary", sixteen_across))

    def eighteen_across(d):
        lit = dw.spread(270, [97, 256, 257], [1, 2, 2])
        syms = [(18, 97 - 11), (1, None), (18, 138 - 11), (18, 20 - 11), (2, None), (2, None), (18, 24 - 11), (1, None), (1, None)]
        assert dw.expand(syms) == lit + [0] * 12 + [1, 1]
        tokens = [97] * 200 + [Match(257, 0, 12, 0), Match(257, 0, 13, 31), 97]
        d.dynamic(1, lit, [0] * 12 + [1, 1], tokens, header=dict(cl_syms=syms))
        return dw.model(tokens)
    out.append(_one("header: an 18 across the literal/distance boundary", eighteen_across))

    def empty_block(d):                                 # a literal/length set that is one 1-bit code, for 256
        d.dynamic(0, dw.spread(257, [256], [1]), [0], [])
        d.stored(0, b"between")
        d.dynamic(1, dw.spread(257, [256], [1]), [0], [])
        return b"between"
    out.append(_one("header: empty blocks of a single 1-bit code", empty_block))

    def empty_member(d):
        d.dynamic(1, dw.spread(257, [256], [1]), [0], [])
        return b""
    out.append(_one("header: a member that is one empty dynamic block", empty_member))
    return out


# ------------------------------------------------------------------------------------------------ 6. block sequences
NINE_BIT = list(range(144, 152))                        # fixed-code literals of 9 bits: 3 + 9 j + 7 bits per block


def _sequences():
    out = []
    text = _noise(50, 61) * 8

    def mixed(d):
        a, b = text[:100], text[100:150]
        t1 = dw.tokens_of(text[150:260], a)
        t2 = dw.tokens_of(text[260:400], a + text[150:260])
        d.stored(0, a)
        d.fixed(0, t1)
        d.dynamic(0, dw.spread(286, _shuffled(range(286), 62), dw.complete_lens(286, 12)), dw.complete_lens(30, 8), t2)
        d.stored(0, b"")
        d.stored(1, b)
        return a + text[150:400] + b
    out.append(_one("sequence: stored, fixed, dynamic, empty stored, stored", mixed))

    def alignments(d):                                  # the stored header's 3 bits begin at bit 2 + j of a byte
        piece = b""
        for j in range(8):
            d.fixed(0, NINE_BIT[:j])
            assert d.sink.bitpos % 8 == (2 + j) % 8
            d.stored(int(j == 7), bytes([j]) * (j + 1))
            piece += bytes(NINE_BIT[:j]) + bytes([j]) * (j + 1)
        return piece
    out.append(_one("sequence: stored blocks at every bit alignment", alignments))

    def largest_stored(d):                              # BSIZE has 16 bits: 65 505 bytes is what a member has room for
        big = _noise(65505, 63)
        d.stored(1, big)
        return big
    out.append(_one("sequence: the largest stored block a member holds", largest_stored))

    def last_bit(d):                                    # 3 + 6 x 9 + 7 = 64 bits
        d.fixed(1, NINE_BIT[:6])
        assert d.sink.bitpos == 64
        return bytes(NINE_BIT[:6])
    out.append(_one("sequence: the last bit of the final block is the last bit of the input", last_bit))

    parts = []
    for k in range(1, 5):
        d = Deflate()
        d.fixed(1, [1, 2, 3, (5, 2), k])
        parts.append((d.raw() + b"\xff\x00\x07\xaa"[:k], dw.model([1, 2, 3, (5, 2), k])))
        d = Deflate()
        d.stored(1, bytes([k]) * 9)
        parts.append((d.raw() + b"\x01\xff\xff\xff"[:k], bytes([k]) * 9))
    out.append(Legal("sequence: 1 to 4 unused bytes behind the final block", parts))

    def across(d):                                      # matches that begin in the block before
        a = _noise(300, 64)
        t1 = [Match(285, 0, 16, 10), (40, 300)]
        mid = dw.model(t1, a)
        t2 = [(258, 2), (100, 300 + len(mid)), Match(270, 1, 17, 3), 7]
        d.stored(0, a)
        d.dynamic(0, dw.spread(286, _shuffled(range(286), 65), dw.complete_lens(286, 13)), dw.complete_lens(30, 7), t1)
        d.fixed(1, t2)
        return a + mid + dw.model(t2, a + mid)
    out.append(_one("sequence: matches that reach back into a stored and into a dynamic block", across))

    # deflate data at each of the 4 byte alignments in the file: a member is 31 + n bytes around n stored ones
    parts, at = [], 0
    for k in (2, 3, 0, 1, 1, 3):
        n = (k - at - 18 - 31) % 4 or 4                 # a stored member that moves the next one's data to alignment k
        if (at + 18) % 4 != k:
            d = Deflate()
            d.stored(1, bytes(n))
            parts.append((d.raw(), bytes(n)))
            at += 31 + n
        d = Deflate()
        tokens = dw.tokens_of(text[:200 + at % 7])
        d.dynamic(1, dw.spread(286, _shuffled(range(286), 66 + k), dw.complete_lens(286, 11)), dw.complete_lens(30, 10), tokens)
        parts.append((d.raw(), text[:200 + at % 7]))
        at += 26 + len(parts[-1][0])
    out.append(Legal("sequence: deflate data at every byte alignment of the file", parts))
    return out


def data_alignments(parts):
    """Offset modulo 4 of each member's deflate data in the concatenated file."""
    out, at = [], 0
    for m in members(parts):
        out.append((at + 18) % 4)
        at += len(m)
    return out


@functools.lru_cache(maxsize=None)
def legal_cases():
    return ([_deep_trees()] + _table_edges() + [_every_symbol(False, 31), _every_symbol(True, 35), _overlaps()]
            + _header_shapes() + _sequences())


# ------------------------------------------------------------------------------------------------ refusals
def _refusals():
    out = []
    abc = [97, 98, 99, 97, 97, 98]

    def add(name, message, build, piece=b""):
        d = Deflate()
        got = build(d)
        out.append(Refusal(name, d.raw(), piece if got is None else got, message))

    def lenient(lit, dist, tokens, header=None):
        def build(d):
            d.dynamic(1, lit, dist, tokens, header=header)
            return dw.model(tokens)
        return build

    small = _small_lit(258, [257])                      # a, b: 2 bits; c, 256, 257: 2 3 3
    add("over-subscribed literal/length set", "invalid literal/lengths set",
        lenient(dw.spread(258, [97, 98, 99, 100, 256], [2, 2, 2, 2, 2]), [1, 1], abc))
    add("over-subscribed distance set", "invalid distances set", lenient(small, [1, 1, 1], abc + [(3, 1)]))
    add("over-subscribed code-length set", "invalid code lengths set",
        lenient(small, [1, 1], abc, dict(cl_lens=dw.spread(19, [0, 1, 2, 3, 17, 18], [2, 2, 2, 2, 2, 2]))))
    add("incomplete literal/length set, longest code 3 bits", "invalid literal/lengths set",
        lenient(dw.spread(258, [97, 98, 99, 256], [2, 2, 3, 3]), [1, 1], abc))
    add("incomplete distance set, longest code 2 bits", "invalid distances set", lenient(small, [2, 2, 2], abc + [(3, 1), (3, 2)]))
    add("incomplete code-length set", "invalid code lengths set",
        lenient(small, [1, 1], abc, dict(cl_lens=dw.spread(19, [0, 1, 2, 3, 17, 18], [2, 2, 3, 3, 3, 4]))))
    add("incomplete code-length set: a single 1-bit code", "invalid code lengths set",
        lambda d: d.dynamic(1, [8] * 257, [8], [], header=dict(cl_lens=dw.spread(19, [8], [1]), cl_syms=[(8, None)] * 258),
                            end=False))
    add("16 as the first code-length symbol", "invalid bit length repeat",
        lenient(small, [1, 1], [], dict(cl_lens=dw.flat_code([0, 1, 2, 3, 16, 18]), cl_syms=[(16, 0)] + dw.run_length(small + [1, 1])[1:])))
    add("a repeat past HLIT + HDIST", "invalid bit length repeat",
        lenient(small, [1, 1], abc, dict(cl_lens=dw.flat_code([0, 1, 2, 3, 16, 17, 18]),
                                        cl_syms=dw.run_length(small + [1])[:-1] + [(1, None), (16, 0)])))
    add("length 0 for symbol 256", "missing end-of-block",
        lambda d: d.dynamic(1, dw.spread(258, [97, 98, 99, 257], [2, 2, 2, 2]), [1, 1], abc, end=False), dw.model(abc))
    add("HCLEN 4: no length but 0 can be named", "missing end-of-block",
        lambda d: d.dynamic(1, [0] * 257, [0], [], header=dict(cl_lens=dw.spread(19, [0, 18], [1, 1]), hclen=4), end=False))
    for hlit in (287, 288):                             # the fields say 287 / 288; the lengths that follow are as many
        lit = dw.spread(hlit, [97, 98, 99, 256], [2, 2, 2, 2])
        add("HLIT %d" % hlit, "too many length or distance symbols", lenient(lit, [1, 1], abc))
    for hdist in (31, 32):
        add("HDIST %d" % hdist, "too many length or distance symbols", lenient(small, dw.spread(hdist, [0, 1], [1, 1]), abc + [(3, 1)]))

    def type3(d):
        d.stored(0, b"before")
        d.sink.put(1, 1)
        d.sink.put(3, 2)
        d.sink.put(0x5A5A5, 20)
        return b"before"
    add("block type 3", "invalid block type", type3)
    for sym in (286, 287):
        add("fixed-code symbol %d" % sym, "invalid literal/length code",
            lambda d, sym=sym: d.fixed(1, abc + [Sym(sym), Dist(0, 0)]), dw.model(abc))
    for dsym in (30, 31):
        add("fixed distance code %d" % dsym, "invalid distance code",
            lambda d, dsym=dsym: d.fixed(1, abc + [Sym(257), Dist(dsym, 0)]), dw.model(abc))
    add("a distance one byte before the start of the output", "invalid distance too far back",
        lambda d: d.fixed(1, abc + [(3, 7), 99]), dw.model(abc) + b"\0ab" + b"c")
    add("a distance code in a block that has none", "invalid distance code",
        lambda d: d.dynamic(1, small, [0], abc + [Sym(257), Bits(0, 4)]), dw.model(abc))
    add("a distance code the incomplete 1-bit set lacks", "invalid distance code",
        lambda d: d.dynamic(1, small, [1], abc + [Sym(257), Bits(1, 1), Bits(0, 4)]), dw.model(abc))
    add("a literal/length code the incomplete 1-bit set lacks", "invalid literal/length code",
        lambda d: d.dynamic(1, dw.spread(257, [256], [1]), [0], [Bits(1, 1), Bits(0, 6)], end=False))
    add("stored LEN / NLEN mismatch", "invalid stored block lengths", lambda d: d.stored(1, b"hello", nlength=5 ^ 0xFFFE), b"hello")
    add("a stored LEN past the input", None, lambda d: d.stored(1, b"hello", length=600), b"hello" + bytes(595))
    # a short dynamic header, cut behind every byte (the whole stream is the first case's member of "header shapes")
    d = Deflate()
    d.dynamic(1, _small_lit(257), [0], abc)
    whole = d.raw()
    assert zlib.decompress(whole, -15) == dw.model(abc)
    for n in range(len(whole)):
        out.append(Refusal("a dynamic block cut to %d of %d bytes" % (n, len(whole)), whole[:n], dw.model(abc), None))
    return out


@functools.lru_cache(maxsize=None)
def refusal_cases():
    return _refusals()


def zlib_verdict(raw):
    """(bytes, None) when zlib inflates `raw` to its end into at most 65 536 bytes; (None, message) when it refuses;
    (None, None) when it wants more input or has more output than a member holds: such a stream is left out."""
    z = zlib.decompressobj(-15)
    try:
        out = z.decompress(raw, 65537)
    except zlib.error as e:
        return None, str(e).split(": ", 1)[1]
    if z.eof and len(out) <= 65536:
        return out, None
    return None, None


# ------------------------------------------------------------------------------------------------ mutants
HEADER_AND_DISTANCE_MESSAGES = (
    "invalid block type", "invalid stored block lengths", "too many length or distance symbols", "invalid code lengths set",
    "invalid bit length repeat", "invalid code -- missing end-of-block", "invalid literal/lengths set", "invalid distances set",
    "invalid literal/length code", "invalid distance code", "invalid distance too far back")
FLIP_BYTES = 110


def _low_entropy(n, seed):
    rng = np.random.RandomState(seed)
    words = [b"chr", b"read", b"\x00\x00\x00", b"ACGT", b"\xff\xff", b"NM", b"quality", b"\x10\x20\x30"]
    return b"".join(words[i] + bytes([j]) for i, j in zip(rng.randint(0, len(words), n // 4), rng.randint(0, 9, n // 4)))[:n]


def _level9(piece, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(piece) + c.flush()


Corpus = namedtuple("Corpus", "accepted refused left_out")


@functools.lru_cache(maxsize=None)
def corpus():
    """Every single-bit flip in the first FLIP_BYTES bytes of three level-9 zlib streams (two dynamic, one of the fixed
    code), sorted by zlib: accepted [(raw, bytes)], refused [(raw, message, the unflipped stream's bytes)], left_out [raw]."""
    accepted, refused, left_out = [], [], []
    for piece, strategy in ((_low_entropy(3000, 71), zlib.Z_DEFAULT_STRATEGY), (_low_entropy(2000, 72) + bytes(600), zlib.Z_DEFAULT_STRATEGY),
                            (bytes(600) + _low_entropy(1500, 73), zlib.Z_FIXED)):
        raw = _level9(piece, strategy)
        assert len(raw) > 2 * FLIP_BYTES
        for bit in range(8 * FLIP_BYTES):
            bad = bytearray(raw)
            bad[bit >> 3] ^= 1 << (bit & 7)
            bad = bytes(bad)
            out, message = zlib_verdict(bad)
            if out is not None:
                accepted.append((bad, out))
            elif message is not None:
                refused.append((bad, message, piece))
            else:
                left_out.append(bad)
    return Corpus(accepted, refused, left_out)


# ------------------------------------------------------------------------------------------------ a BAM by the writer
def bgzf_by_writer(data, seed, eof_block=b""):
    """`data` as BGZF members cut at seeded offsets, every member 1 to 4 deflate blocks of a seeded mix of stored, fixed
    and deep-tree dynamic blocks (the commonest bytes on the 15-bit codes); matches reach back across the blocks."""
    rng = np.random.RandomState(seed)
    order = [int(s) for s in np.argsort(-np.bincount(np.frombuffer(data, np.uint8), minlength=256), kind="stable")]
    lens = dw.complete_lens(286, 15, deep=True)[::-1]
    lit = dw.spread(286, order[:128] + [256] + list(range(257, 286)) + order[128:], lens)
    dist = dw.spread(30, _shuffled(range(30), seed), dw.complete_lens(30, 15, deep=True))
    out, at = [], 0
    while at < len(data):
        piece = data[at:at + int(rng.randint(1, 24000))]
        at += len(piece)
        d = Deflate()
        cuts = sorted(set([0, len(piece)] + [int(c) for c in rng.randint(0, len(piece) + 1, int(rng.randint(0, 4)))]))
        for a, b in zip(cuts[:-1], cuts[1:]):
            kind, last = int(rng.randint(0, 3)), int(b == len(piece))
            if kind == 0:
                d.stored(last, piece[a:b])
            elif kind == 1:
                d.fixed(last, dw.tokens_of(piece[a:b], piece[:a]))
            else:
                d.dynamic(last, lit, dist, dw.tokens_of(piece[a:b], piece[:a]))
        out.append(dw.member(piece, d.raw()))
    return b"".join(out) + eof_block


# ------------------------------------------------------------------------------------------------ the scanner
def _table(lens):
    """2^15 entries (symbol, length) by the next 15 bits, least significant first; None where no code begins."""
    table = [None] * 32768
    for sym, c in enumerate(dw.canonical(lens)):
        if c is None:
            continue
        code, l = c
        rev = int(format(code, "0%db" % l)[::-1], 2)
        table[rev::1 << l] = [(sym, l)] * (32768 >> l)
    return table


class ScanError(Exception):
    pass


def scan(raw):
    """A plain inflate of `raw` that reports what it had to do: (blocks, output, bits used).  Per block a dict: type, last,
    start (bit offset of its header); for Huffman blocks lit_max / dist_max (longest code of the set), lit_by_len /
    dist_by_len (decoded symbols by code length), matches (Counter of (lsym, lextra, dsym, dextra)), lit_lens / dist_lens,
    out_start (output bytes before the block), sources (where the matches that begin before out_start begin); for dynamic ones
    hlit, hdist, hclen, cl_lens, cl_syms [(position in the length list, symbol, extra)].  Raises ScanError where it cannot
    go on: it is no judge of legality, zlib is."""
    data = bytes(raw) + bytes(16)
    pos, out, blocks = 0, bytearray(), []

    def peek(n):
        return (int.from_bytes(data[pos >> 3:(pos >> 3) + 8], "little") >> (pos & 7)) & ((1 << n) - 1)

    def take(n):
        nonlocal pos
        v = peek(n)
        pos += n
        if pos > 8 * len(raw):
            raise ScanError("past the end")
        return v

    def symbol(table):
        nonlocal pos
        e = table[peek(15)]
        if e is None:
            raise ScanError("no such code")
        pos += e[1]
        if pos > 8 * len(raw):
            raise ScanError("past the end")
        return e

    while True:
        b = dict(start=pos, last=take(1), type=take(2))
        blocks.append(b)
        if b["type"] == 0:
            pos = (pos + 7) & ~7
            n, c = take(16), take(16)
            if n ^ 0xFFFF != c or (pos >> 3) + n > len(raw):
                raise ScanError("stored lengths")
            out += raw[pos >> 3:(pos >> 3) + n]
            pos += 8 * n
            b["stored"] = n
        elif b["type"] == 3:
            raise ScanError("type 3")
        else:
            if b["type"] == 1:
                lit_lens, dist_lens = dw.FIXED_LIT, dw.FIXED_DIST
            else:
                b["hlit"], b["hdist"], b["hclen"] = take(5) + 257, take(5) + 1, take(4) + 4
                cl = [0] * 19
                for i in range(b["hclen"]):
                    cl[dw.CL_ORDER[i]] = take(3)
                b["cl_lens"], b["cl_syms"] = cl, []
                table, lens = _table(cl), []
                while len(lens) < b["hlit"] + b["hdist"]:
                    s, _ = symbol(table)
                    extra = take({16: 2, 17: 3, 18: 7}[s]) if s >= 16 else None
                    b["cl_syms"].append((len(lens), s, extra))
                    if s == 16 and not lens:
                        raise ScanError("16 first")
                    lens += dw.expand([(lens[-1], None), (16, extra)])[1:] if s == 16 else dw.expand([(s, extra)])
                if len(lens) > b["hlit"] + b["hdist"]:
                    raise ScanError("repeat past the end")
                lit_lens, dist_lens = lens[:b["hlit"]], lens[b["hlit"]:]
            b["lit_lens"], b["dist_lens"], b["out_start"], b["sources"] = list(lit_lens), list(dist_lens), len(out), []
            b["lit_max"], b["dist_max"] = max(lit_lens), max(dist_lens)
            b["lit_by_len"], b["dist_by_len"], b["matches"] = Counter(), Counter(), Counter()
            lit, dist = _table(lit_lens), _table(dist_lens)
            while True:
                s, l = symbol(lit)
                b["lit_by_len"][l] += 1
                if s < 256:
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise ScanError("symbol %d" % s)
                le = take(dw.LEN_EXTRA[s - 257])
                ds, l = symbol(dist)
                if ds > 29:
                    raise ScanError("distance symbol %d" % ds)
                b["dist_by_len"][l] += 1
                de = take(dw.DIST_EXTRA[ds])
                b["matches"][(s, le, ds, de)] += 1
                length, distance = dw.LEN_BASE[s - 257] + le, dw.DIST_BASE[ds] + de
                if distance > len(out):
                    raise ScanError("too far back")
                if len(out) - distance < b["out_start"]:
                    b["sources"].append(len(out) - distance)
                if distance >= length:
                    out += out[len(out) - distance:len(out) - distance + length]
                else:
                    for _ in range(length):
                        out.append(out[-distance])
        if b["last"]:
            return blocks, bytes(out), pos


def reach(blocks):
    """What a list of scanned blocks makes the kernel's decoder do: the longest literal/length and distance code among the
    sets, the longest ones decoded, and how many symbols were decoded beyond the table widths."""
    r = dict(lit_max=0, dist_max=0, lit_used=0, dist_used=0, lit_slow=0, dist_slow=0)
    for b in blocks:
        if b["type"] == 0:
            continue
        r["lit_max"], r["dist_max"] = max(r["lit_max"], b["lit_max"]), max(r["dist_max"], b["dist_max"])
        r["lit_used"] = max([r["lit_used"]] + list(b["lit_by_len"]))
        r["dist_used"] = max([r["dist_used"]] + list(b["dist_by_len"]))
        r["lit_slow"] += sum(n for l, n in b["lit_by_len"].items() if l > LIT_BITS)
        r["dist_slow"] += sum(n for l, n in b["dist_by_len"].items() if l > DIST_BITS)
    return r
