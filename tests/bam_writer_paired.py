"""BAM records with a flag word and a mate position for the paired-mode tests (tests/bam_writer.py::record always writes
mate position -1); the BGZF framing is bam_writer's."""
import struct

import numpy as np

from bam_writer import bgzf


def record(ref_id, pos, mapq, flag, mate_pos, name=b"r", n_cigar=1, l_seq=10, tags=b"", mate_ref=None):
    name_z = name + b"\0"
    cigar = struct.pack("<%dI" % n_cigar, *([(max(l_seq, 1) << 4) | 0] * n_cigar))
    body = struct.pack("<iiBBHHHiiii", ref_id, pos, len(name_z), mapq, 4680, n_cigar, flag, l_seq,
                       ref_id if mate_ref is None else mate_ref, mate_pos, 0)
    body += name_z + cigar + bytes((l_seq + 1) // 2) + b"\xff" * l_seq + tags
    return struct.pack("<i", len(body)) + body


def plain_bam(refs, records, text=b"@HD\tVN:1.6\tSO:coordinate\n"):
    """The uncompressed BAM stream: refs = [(name, length)], records = [(ref_id, pos, mapq, flag, mate_pos)] in file
    order; names, CIGAR counts, sequence lengths and tags vary with the record number."""
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(refs))]
    for name, length in refs:
        nm = name.encode() + b"\0"
        out += [struct.pack("<i", len(nm)), nm, struct.pack("<i", int(length))]
    for i, (ref_id, pos, mapq, flag, mate_pos) in enumerate(records):
        out.append(record(int(ref_id), int(pos), int(mapq), int(flag), int(mate_pos), name=b"read%d" % i * (1 + i % 3),
                          n_cigar=i % 4, l_seq=(i * 7) % 60, tags=b"NMC\x01" * (i % 3)))
    return b"".join(out)


def write_bam(path, refs, records, cuts=None, eof=True, seed=None):
    data = plain_bam(refs, records)
    if seed is not None:
        rng = np.random.RandomState(seed)
        cuts = sorted(rng.randint(1, len(data), size=max(2, len(data) // 3000)).tolist())
    with open(path, "wb") as f:
        f.write(bgzf(data, cuts, eof))
    return data


def records_of(ref_ids, pos_by_ref, mapq_by_ref, flag_by_ref, mate_by_ref, unplaced=0):
    """File-order records from per-reference arrays, then `unplaced` reads without coordinates."""
    recs = []
    for ref_id, pos, mapq, flag, mate in zip(ref_ids, pos_by_ref, mapq_by_ref, flag_by_ref, mate_by_ref):
        recs += [(ref_id, int(p), int(q), int(f), int(m)) for p, q, f, m in zip(pos, mapq, flag, mate)]
    recs += [(-1, -1, 0, 0x4 | 0x1, -1)] * unplaced
    return recs
