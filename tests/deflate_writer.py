"""A bit-level deflate writer for the tests (plain Python, RFC 1951): stored, fixed and dynamic blocks from a list of
tokens, with the dynamic header under the caller's control (HLIT / HDIST / HCLEN as raw fields, the code-length code's own
lengths, the exact sequence of code-length symbols with their 16 / 17 / 18 repeats) and raw tokens that put an arbitrary
symbol number or field value into the stream.  It writes what no encoder writes: legal streams zlib never produces and
streams every decoder must refuse.  `model(tokens)` gives the bytes a token list stands for.

Tokens: an int is a literal; a pair (length, distance) is a match in its usual encoding (258 as symbol 285);
Match(lsym, lextra, dsym, dextra) names the two symbols and their extra-bit values; Sym(n) / Dist(n, extra) put one
symbol of the literal/length / distance code (any number that has a code, legal or not); Bits(value, n) puts a field."""
import struct
import zlib
from collections import namedtuple

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32

Match = namedtuple("Match", "lsym lextra dsym dextra")
Sym = namedtuple("Sym", "n")
Dist = namedtuple("Dist", "n extra")
Bits = namedtuple("Bits", "value n")


class BitSink:
    """Bytes from bits: fields least significant bit first, Huffman codes most significant bit first."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, value, nbits):
        self.put(int(format(value, "0%db" % nbits)[::-1], 2) if nbits else 0, nbits)

    @property
    def bitpos(self):
        return 8 * len(self.out) + self.n

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self, raw):
        assert self.n == 0
        self.out += raw

    def done(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """(code, length) per symbol, None where the length is 0: the canonical assignment of RFC 1951, 3.2.2.  Over-subscribed
    sets get codes too (cut to their length): the refusals need something to write."""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(None)
        else:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
    return out


def kraft(lens):
    """Sum of 2^-length in units of 2^-15: 32768 for a complete set."""
    return sum(1 << (15 - l) for l in lens if l)


def complete_lens(n, maxlen, deep=False):
    """The sorted lengths of a complete code of n symbols whose longest code has exactly maxlen bits: the chain
    1, 2, .., maxlen - 1, maxlen, maxlen with one leaf split in two until n are there, the shortest leaf first (most
    codes short) or, `deep`, the longest one below maxlen first (most codes long)."""
    assert maxlen + 1 <= n <= (1 << maxlen)
    count = [0] * (maxlen + 1)
    for l in range(1, maxlen):
        count[l] = 1
    count[maxlen] = 2
    for _ in range(n - maxlen - 1):
        order = range(maxlen - 1, 0, -1) if deep else range(1, maxlen)
        l = next(l for l in order if count[l])
        count[l] -= 1
        count[l + 1] += 2
    out = [l for l in range(1, maxlen + 1) for _ in range(count[l])]
    assert len(out) == n and kraft(out) == 32768 and out[-1] == maxlen
    return out


def spread(n, symbols, lengths):
    """A length list of n entries: symbols[i] gets lengths[i], every other symbol 0."""
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    assert len(symbols) == len(lengths) == len(set(symbols))
    return out


def length_token(length):
    """(symbol, extra) of a match length in its usual encoding."""
    if length == 258:
        return 285, 0
    s = max(i for i in range(28) if LEN_BASE[i] <= length)
    return 257 + s, length - LEN_BASE[s]


def distance_token(distance):
    s = max(i for i in range(30) if DIST_BASE[i] <= distance)
    return s, distance - DIST_BASE[s]


def explicit(token):
    """A match token as Match(lsym, lextra, dsym, dextra)."""
    if isinstance(token, Match):
        return token
    return Match(*(length_token(token[0]) + distance_token(token[1])))


def model(tokens, before=b""):
    """The bytes `tokens` stand for, behind `before` (what the member has put out so far; not returned)."""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
            continue
        assert not isinstance(t, (Sym, Dist, Bits)), "raw tokens have no model"
        m = explicit(t)
        length, dist = LEN_BASE[m.lsym - 257] + m.lextra, DIST_BASE[m.dsym] + m.dextra
        assert 3 <= length <= 258 and 1 <= dist <= len(out)
        for _ in range(length):
            out.append(out[-dist])
    return bytes(out[len(before):])


def run_length(lens):
    """Code-length symbols for `lens` as (symbol, extra): the plain greedy use of 16 / 17 / 18 within one list."""
    out, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                out.append((18, k - 11))
                run -= k
            if run >= 3:
                out.append((17, run - 3))
                run = 0
            out += [(0, None)] * run
        else:
            out.append((v, None))
            run -= 1
            while run >= 3:
                k = min(run, 6)
                out.append((16, k - 3))
                run -= k
            out += [(v, None)] * run
        i = j
    return out


def expand(cl_syms):
    """The lengths a sequence of code-length symbols stands for."""
    out = []
    for s, extra in cl_syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + extra)
        else:
            out += [0] * ((3 if s == 17 else 11) + extra)
    return out


def flat_code(used, n=19):
    """Lengths of a complete code over the symbols `used` (of n), as even as a complete code can be; a lone symbol
    gets a partner, since a single code is an incomplete set."""
    used = sorted(set(used))
    if len(used) == 1:
        used = sorted(set(used + [0 if used[0] else 1]))
    k = len(used)
    top = max(1, (k - 1).bit_length())
    short = (1 << top) - k
    return spread(n, used, [top - 1] * short + [top] * (k - short))


class Deflate:
    """One raw deflate stream, block by block.  `raw()` ends it (padded to the byte with zero bits)."""

    def __init__(self):
        self.sink = BitSink()

    def raw(self):
        return self.sink.done()

    def stored(self, last, payload, length=None, nlength=None):
        """LEN / NLEN may be given as raw fields for the refusals."""
        s = self.sink
        s.put(last, 1)
        s.put(0, 2)
        s.align()
        length = len(payload) if length is None else length
        s.bytes(struct.pack("<HH", length, (length ^ 0xFFFF) if nlength is None else nlength) + bytes(payload))

    def fixed(self, last, tokens, end=True):
        self.sink.put(last, 1)
        self.sink.put(1, 2)
        self._tokens(tokens, canonical(FIXED_LIT), canonical(FIXED_DIST), end)

    def dynamic(self, last, lit_lens, dist_lens, tokens, header=None, end=True):
        """header: any of hlit / hdist (the raw 5-bit fields), hclen (4..19), cl_lens (the 19 lengths of the code-length
        code, by symbol), cl_syms (the code-length symbols as (symbol, extra)); what is missing is derived."""
        h = dict(header or {})
        s = self.sink
        lit_lens, dist_lens = list(lit_lens), list(dist_lens)
        cl_syms = h.get("cl_syms")
        if cl_syms is None:
            cl_syms = run_length(lit_lens + dist_lens)
        cl_lens = h.get("cl_lens")
        if cl_lens is None:
            cl_lens = flat_code([c for c, _ in cl_syms])
        hclen = h.get("hclen")
        if hclen is None:
            hclen = max([4] + [i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]])
        assert 4 <= hclen <= 19 and len(cl_lens) == 19
        s.put(last, 1)
        s.put(2, 2)
        s.put(h.get("hlit", len(lit_lens) - 257), 5)
        s.put(h.get("hdist", len(dist_lens) - 1), 5)
        s.put(hclen - 4, 4)
        for i in range(hclen):
            s.put(cl_lens[CL_ORDER[i]], 3)
        codes = canonical(cl_lens)
        for c, extra in cl_syms:
            s.code(*codes[c])
            if c >= 16:
                s.put(extra, {16: 2, 17: 3, 18: 7}[c])
        self._tokens(tokens, canonical(lit_lens), canonical(dist_lens), end)

    def _tokens(self, tokens, lit, dist, end):
        s = self.sink
        for t in tokens:
            if isinstance(t, int):
                s.code(*lit[t])
            elif isinstance(t, Sym):
                s.code(*lit[t.n])
            elif isinstance(t, Dist):
                s.code(*dist[t.n])
                s.put(t.extra, DIST_EXTRA[t.n] if t.n < 30 else 0)
            elif isinstance(t, Bits):
                s.put(t.value, t.n)
            else:
                m = explicit(t)
                s.code(*lit[m.lsym])
                s.put(m.lextra, LEN_EXTRA[m.lsym - 257])
                s.code(*dist[m.dsym])
                s.put(m.dextra, DIST_EXTRA[m.dsym])
        if end:
            s.code(*lit[256])


def member(piece, cdata, crc=None, isize=None):
    """One BGZF member around raw deflate data: the `_block` of test_bamgpu_gpu.py, restated."""
    assert len(cdata) + 25 < 65536 and len(piece) <= 65536
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cdata) + 25) + cdata
            + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF if crc is None else crc, len(piece) if isize is None else isize))


def tokens_of(data, before=b"", shortest=4):
    """A plain greedy LZ77 parse of `data` (3-byte hash, last occurrence, window 32 768): tokens whose matches may reach
    back into `before`.  Not a good encoder; the tests need streams with matches in them, not small ones."""
    buf = bytes(before) + bytes(data)
    at, seen, out = len(before), {}, []
    for i in range(max(0, len(before) - 32768), max(0, len(before) - 2)):
        seen[buf[i:i + 3]] = i
    while at < len(buf):
        key = buf[at:at + 3]
        prev = seen.get(key) if len(key) == 3 else None
        if prev is not None and at - prev <= 32768:
            n = 3
            while n < 258 and at + n < len(buf) and buf[prev + n] == buf[at + n]:
                n += 1
            if n >= shortest:
                out.append((n, at - prev))
                for j in range(at, min(at + n, len(buf) - 2)):
                    seen[buf[j:j + 3]] = j
                at += n
                continue
        if len(key) == 3:
            seen[key] = at
        out.append(buf[at])
        at += 1
    return out
