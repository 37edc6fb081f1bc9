"""A small PDF reader for the tests of `plotpdf`: it follows startxref, the classic xref table and the objects, resolves
an indirect /Length, inflates a FlateDecode stream, tokenises a content stream and interprets exactly the operators this
build emits (q Q re W n f S m l w rg RG gs cs scn BT ET Tf Td Tj); anything else raises.  tests/test_pdf_cases_cpu.py
first proves it on a file that matplotlib's PDF backend writes."""
import re
import zlib

WHITE = b" \t\r\n\x0c\x00"
DELIM = b"()<>[]{}/%"


class Ref(object):
    def __init__(self, num, gen):
        self.num, self.gen = num, gen

    def __repr__(self):
        return "%d %d R" % (self.num, self.gen)


class Name(str):
    pass


class Op(str):
    pass


def _skip(data, at):
    while at < len(data):
        if data[at] in WHITE:
            at += 1
        elif data[at:at + 1] == b"%":
            while at < len(data) and data[at] not in b"\r\n":
                at += 1
        else:
            break
    return at


def parse(data, at):
    """One object (or a bare keyword, as an Op) at `at`: (value, position behind it)."""
    at = _skip(data, at)
    c = data[at:at + 1]
    if c == b"/":
        end = at + 1
        while end < len(data) and data[end] not in WHITE and data[end] not in DELIM:
            end += 1
        return Name(data[at + 1:end].decode("latin1")), end
    if data[at:at + 2] == b"<<":
        out, at = {}, at + 2
        while True:
            at = _skip(data, at)
            if data[at:at + 2] == b">>":
                return out, at + 2
            key, at = parse(data, at)
            assert isinstance(key, Name), key
            out[key], at = parse(data, at)
    if c == b"<":
        end = data.index(b">", at)
        digits = re.sub(rb"\s", b"", data[at + 1:end])
        assert re.match(rb"^[0-9A-Fa-f]*$", digits), digits
        return bytes.fromhex((digits + (b"0" if len(digits) % 2 else b"")).decode()), end + 1
    if c == b"[":
        out, at = [], at + 1
        while True:
            at = _skip(data, at)
            if data[at:at + 1] == b"]":
                return out, at + 1
            value, at = parse(data, at)
            out.append(value)
    if c == b"(":
        depth, end, out = 1, at + 1, bytearray()
        while depth:
            ch = data[end]
            if ch == 0x5c:
                out.append(data[end + 1])           # (escapes other than \( \) \\ do not occur in what is read here)
                end += 2
                continue
            depth += (ch == 0x28) - (ch == 0x29)
            if depth:
                out.append(ch)
            end += 1
        return bytes(out), end
    end = at
    while end < len(data) and data[end] not in WHITE and data[end] not in DELIM:
        end += 1
    token = data[at:end]
    assert token, (at, data[at:at + 20])
    if re.match(rb"^[+-]?\d+$", token):
        # an indirect reference: integer integer R
        m = re.match(rb"\s+(\d+)\s+R(?![^\s()<>\[\]{}/%])", data[end:end + 32])
        if m and not token.startswith((b"+", b"-")):
            return Ref(int(token), int(m.group(1))), end + m.end()
        return int(token), end
    if re.match(rb"^[+-]?(\d+\.?\d*|\.\d+)$", token):
        return float(token), end
    return Op(token.decode("latin1")), end


class Document(object):
    def __init__(self, data):
        self.data = data
        assert data.startswith(b"%PDF-1."), data[:8]
        tail = data[-64:]
        assert tail.rstrip().endswith(b"%%EOF"), tail
        m = re.search(rb"startxref\s+(\d+)\s+%%EOF\s*$", data[-64:])
        assert m, tail
        self.startxref = int(m.group(1))
        assert data[self.startxref:self.startxref + 4] == b"xref", data[self.startxref:self.startxref + 8]
        self.offsets = {}
        at = _skip(data, self.startxref + 4)
        while data[at:at + 7] != b"trailer":
            first, at = parse(data, at)
            count, at = parse(data, at)
            at = _skip(data, at)
            for i in range(count):
                entry = data[at + 20 * i:at + 20 * i + 20]
                assert re.match(rb"^\d{10} \d{5} [nf][ \r][\r\n]$", entry), entry
                if entry[17:18] == b"n":
                    self.offsets[first + i] = int(entry[:10])
            at = _skip(data, at + 20 * count)
        self.trailer, _ = parse(data, at + 7)
        self.cache = {}

    def obj(self, num):
        """(value, stream bytes or None) of object `num`; the xref offset must land on its 'num gen obj'."""
        if num not in self.cache:
            at = self.offsets[num]
            m = re.match(rb"(\d+)\s+(\d+)\s+obj", self.data[at:at + 32])
            assert m and int(m.group(1)) == num, (num, self.data[at:at + 32])
            value, at = parse(self.data, at + m.end())
            at = _skip(self.data, at)
            stream = None
            if self.data[at:at + 6] == b"stream":
                at += 6
                at += 2 if self.data[at:at + 2] == b"\r\n" else 1
                length = self.get(value[Name("Length")])
                stream = self.data[at:at + length]
                assert len(stream) == length
                assert self.data[_skip(self.data, at + length):][:9] == b"endstream", self.data[at + length:at + length + 16]
            else:
                assert self.data[at:at + 6] == b"endobj", self.data[at:at + 16]
            self.cache[num] = (value, stream)
        return self.cache[num]

    def get(self, value):
        while isinstance(value, Ref):
            value = self.obj(value.num)[0]
        return value

    def stream(self, ref):
        """The decoded bytes of a stream object."""
        value, raw = self.obj(ref.num)
        assert raw is not None
        filt = self.get(value.get(Name("Filter")))
        if filt is None:
            return raw
        assert filt == "FlateDecode" or filt == ["FlateDecode"], filt
        return zlib.decompress(raw)

    def page(self, index=0):
        """(page dictionary with /MediaBox and /Resources inherited, content bytes)."""
        node = self.get(self.get(self.trailer[Name("Root")])[Name("Pages")])
        inherited = {}
        while node.get(Name("Type")) == "Pages":
            for key in ("MediaBox", "Resources"):
                if Name(key) in node:
                    inherited[Name(key)] = node[Name(key)]
            node = self.get(self.get(node[Name("Kids")])[index])
            index = 0
        page = dict(inherited)
        page.update(node)
        contents = page[Name("Contents")]
        resolved = self.get(contents)
        refs = resolved if isinstance(resolved, list) else [contents]
        return page, b"\n".join(self.stream(r) for r in refs)


def tokenize(content):
    """[(operands, operator)] of a content stream."""
    out, operands, at = [], [], _skip(content, 0)
    while at < len(content):
        value, at = parse(content, at)
        if isinstance(value, Op):
            out.append((operands, str(value)))
            operands = []
        else:
            operands.append(value)
        at = _skip(content, at)
    assert not operands, operands
    return out


def cents(v):
    return int(round(float(v) * 100))


def interpret(content, doc=None, resources=None):
    """The drawing a content stream of this build makes: a list of dicts
      fill    rect (x, y, w, h) in centipoints, rgb (hundredths) or pattern (name), a8, clip
      stroke  path [('m' | 'l', x, y) | ('re', x, y, w, h)], rgb, width (hundredths of a point), a8, clip
      text    x, y, size, text, rgb, a8, clip
    An operator outside the set this build emits raises ValueError."""
    state = dict(fill=(0, 0, 0), stroke=(0, 0, 0), pattern=None, width=100, a8=255, clip=None)
    stack, path, out = [], [], []
    pending_clip = False
    text = None
    gstates = {}
    if doc is not None and resources is not None:
        gstates = doc.get(doc.get(resources).get(Name("ExtGState"), {}))
    for operands, op in tokenize(content):
        if op == "q":
            stack.append(dict(state))
        elif op == "Q":
            state = stack.pop()
        elif op == "re":
            path.append(("re",) + tuple(cents(v) for v in operands))
        elif op == "m" or op == "l":
            path.append((op, cents(operands[0]), cents(operands[1])))
        elif op == "W":
            pending_clip = True
        elif op == "n":
            if pending_clip:
                assert len(path) == 1 and path[0][0] == "re", path
                state["clip"] = path[0][1:]
            path, pending_clip = [], False
        elif op == "f":
            assert path and all(seg[0] == "re" for seg in path), path
            for seg in path:
                out.append(dict(kind="fill", rect=seg[1:], rgb=None if state["pattern"] else state["fill"], pattern=state["pattern"],
                                a8=state["a8"], clip=state["clip"]))
            path = []
        elif op == "S":
            if any(seg[0] != "m" for seg in path):
                out.append(dict(kind="stroke", path=path, rgb=state["stroke"], width=state["width"], a8=state["a8"], clip=state["clip"]))
            path = []
        elif op == "w":
            state["width"] = cents(operands[0])
        elif op == "rg":
            state["fill"], state["pattern"] = tuple(cents(v) for v in operands), None
        elif op == "RG":
            state["stroke"] = tuple(cents(v) for v in operands)
        elif op == "gs":
            name = operands[0]
            if gstates:
                entry = doc.get(gstates[name])
                assert entry[Name("ca")] == entry[Name("CA")]
                state["a8"] = int(round(float(entry[Name("ca")]) * 255))
            else:
                assert re.match(r"^A\d{3}$", name), name
                state["a8"] = int(name[1:])
        elif op == "cs":
            assert operands == ["Pattern"], operands
        elif op == "scn":
            state["pattern"] = str(operands[0])
        elif op == "BT":
            text = dict(kind="text", x=0, y=0, size=None, text=b"")
        elif op == "Tf":
            assert operands[0] == "F1"
            text["size"] = operands[1]
        elif op == "Td":
            text["x"], text["y"] = text["x"] + cents(operands[0]), text["y"] + cents(operands[1])
        elif op == "Tj":
            text["text"] += operands[0]
        elif op == "ET":
            text.update(rgb=state["fill"], a8=state["a8"], clip=state["clip"], text=text["text"].decode("latin1"))
            out.append(text)
            text = None
        else:
            raise ValueError("operator %r is not one this build emits" % op)
    assert not stack and not path and text is None
    return out
