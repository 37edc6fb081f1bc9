"""A small BAM writer for the tests (struct + zlib, no htslib): header, records with names / CIGAR / sequence / tags of
varying length, BGZF blocks cut at arbitrary byte positions, the EOF block."""
import struct
import zlib

import numpy as np


def record(ref_id, pos, mapq, flag=0, name=b"r", n_cigar=1, l_seq=10, tags=b""):
    name_z = name + b"\0"
    cigar = struct.pack("<%dI" % n_cigar, *([(max(l_seq, 1) << 4) | 0] * n_cigar))
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name_z), mapq, 4680, n_cigar, flag, l_seq, -1, -1, 0)
    body += name_z + cigar + bytes((l_seq + 1) // 2) + b"\xff" * l_seq + tags
    return struct.pack("<i", len(body)) + body


def plain_bam(refs, records, text=b"@HD\tVN:1.6\tSO:coordinate\n"):
    """The uncompressed BAM stream: refs = [(name, length)], records = [(ref_id, pos, mapq, flag)] in file order;
    names, CIGAR counts, sequence lengths and tags vary with the record number."""
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        nm = name.encode() + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", int(length))]
    for i, (ref_id, pos, mapq, flag) in enumerate(records):
        out.append(record(int(ref_id), int(pos), int(mapq), int(flag), name=b"read%d" % i * (1 + i % 3), n_cigar=i % 4,
                          l_seq=(i * 7) % 60, tags=b"NMC\x01" * (i % 3)))
    return b"".join(out)


def bgzf_block(piece, level=6):
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    cd = c.compress(piece) + c.flush()
    return (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(cd) + 25) + cd
            + struct.pack("<II", zlib.crc32(piece) & 0xFFFFFFFF, len(piece)))


EOF_BLOCK = bgzf_block(b"")


def bgzf(data, cuts=None, eof=True, block=60000, level=6):
    """`data` as BGZF: cut at the byte positions `cuts` (default: every `block` bytes; pieces stay below 64 KiB)."""
    if cuts is None:
        cuts = list(range(block, len(data), block))
    edges = [0] + sorted(set(int(c) for c in cuts if 0 < c < len(data))) + [len(data)]
    out = []
    for a, b in zip(edges[:-1], edges[1:]):
        for s in range(a, b, 65000):
            out.append(bgzf_block(data[s:min(b, s + 65000)], level))
    if eof:
        out.append(EOF_BLOCK)
    return b"".join(out)


def write_bam(path, refs, records, cuts=None, eof=True, seed=None):
    data = plain_bam(refs, records)
    if seed is not None:
        rng = np.random.RandomState(seed)
        cuts = sorted(rng.randint(1, len(data), size=max(2, len(data) // 3000)).tolist())
    with open(path, "wb") as f:
        f.write(bgzf(data, cuts, eof))
    return data


def records_of(ref_ids, pos_by_ref, mapq_by_ref, unplaced=0):
    """File-order records from per-reference arrays; every 11th read secondary (0x100), every 13th flagged unmapped
    (0x4, still placed), then `unplaced` reads without coordinates."""
    recs = []
    for ref_id, pos, mapq in zip(ref_ids, pos_by_ref, mapq_by_ref):
        for p, q in zip(pos, mapq):
            i = len(recs)
            recs.append((ref_id, int(p), int(q), (0x100 if i % 11 == 5 else 0) | (0x4 if i % 13 == 7 else 0)))
    recs += [(-1, -1, 0, 0x4)] * unplaced
    return recs
