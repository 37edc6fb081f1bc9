"""exporttracks restated in plain Python: repr, integer arithmetic, struct, zlib.  Nothing of the product is used here;
CPython's float.__repr__ is the reference for every value, and the BGZF walk follows the SAM specification, section 4.1."""
import math
import struct
import zlib

BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def chrom_ranges(sizes):
    at = 0
    for c, n in enumerate(sizes):
        yield c, at, at + n
        at += n


def track_text(row, sizes, binsize, prefix="chr", clip=None, nozero=False):
    """(bytes, bins left out as not finite): a line per maximal run of bins with the same 64 bits inside a chromosome."""
    lines, dropped = [], 0
    for c, lo, hi in chrom_ranges(sizes):
        a = lo
        while a < hi:
            b = a
            while b + 1 < hi and bits_of(row[b + 1]) == bits_of(row[a]):
                b += 1
            value = float(row[a])
            if not math.isfinite(value):
                dropped += b - a + 1
            elif not (nozero and value == 0.0):
                end = (b - lo + 1) * binsize
                if clip is not None:
                    end = min(end, clip[c])
                lines.append("%s%d\t%d\t%d\t%s\n" % (prefix, c + 1, (a - lo) * binsize, end, repr(value)))
            a = b + 1
    return "".join(lines).encode("ascii"), dropped


def expand(text, binsize, prefix="chr"):
    """{(chromosome from 0, bin): value} of a track's text; raises where a bin is covered twice or a start is no multiple
    of the bin size.  A clipped end counts as the end of the bin it lies in."""
    bins = {}
    for line in text.decode("ascii").splitlines():
        name, start, end, value = line.split("\t")
        assert name.startswith(prefix) and name[len(prefix):].isdigit(), line
        c, start, end = int(name[len(prefix):]) - 1, int(start), int(end)
        assert start % binsize == 0 and end > start, line
        for k in range(start // binsize, (end + binsize - 1) // binsize):
            assert (c, k) not in bins, line
            bins[(c, k)] = float(value)
    return bins


def calls_bed(calls, binsize, prefix="chr", clip=None, mineffect=0):
    """BED9 bytes of the calls [chromosome from 1, first bin, last bin, z, effect]."""
    kept = []
    for at, call in enumerate(calls):
        z, effect = float(call[3]), float(call[4])
        if not abs(effect * 100) > mineffect:
            continue
        chrom, start, end = int(call[0]), int(call[1]) * binsize, (int(call[2]) + 1) * binsize
        if clip is not None:
            end = min(end, clip[chrom - 1])
        if math.isnan(z):
            score = 0
        elif math.isinf(z):
            score = 1000
        else:
            score = min(1000, int(round(abs(z) * 10)))
        fields = ["%s%d" % (prefix, chrom), str(start), str(end), "z=%.2f;effect=%.2f%%" % (z, effect * 100), str(score), ".", str(start),
                  str(end), "213,94,0" if effect > 0 else "0,114,178"]
        kept.append(((chrom, start, end, at), "\t".join(fields) + "\n"))
    return "".join(line for _, line in sorted(kept)).encode("ascii")


def bgzf_blocks(data):
    """[(payload, crc, isize)] of every block of a BGZF byte string, the end-of-file block included as the last; raises
    ValueError on a bad header, on a walk that does not end exactly at the last byte, or on a missing end-of-file block."""
    blocks, at = [], 0
    while at < len(data):
        head = data[at:at + 18]
        if len(head) < 18 or head[:4] != b"\x1f\x8b\x08\x04" or head[10:12] != b"\x06\x00" or head[12:16] != b"BC\x02\x00":
            raise ValueError("bad BGZF header at byte %d" % at)
        size = struct.unpack("<H", head[16:18])[0] + 1
        if size < 26 or at + size > len(data):
            raise ValueError("the block at byte %d has %d bytes, %d are left" % (at, size, len(data) - at))
        crc, isize = struct.unpack("<II", data[at + size - 8:at + size])
        blocks.append((data[at + 18:at + size - 8], crc, isize))
        at += size
    if not blocks or data[-28:] != BGZF_EOF:
        raise ValueError("no end-of-file block")
    return blocks


def bgzf_of(data, block=65280, level=6):
    """`data` as BGZF made with zlib: blocks of `block` input bytes and the end-of-file block."""
    out = []
    for at in range(0, len(data), block):
        piece = data[at:at + block]
        packer = zlib.compressobj(level, zlib.DEFLATED, -15)
        raw = packer.compress(piece) + packer.flush()
        out.append(BGZF_EOF[:16] + struct.pack("<H", len(raw) + 25) + raw + struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out) + BGZF_EOF
