"""The GPU result encoder (csrc/deflate.hip, testbatch -encoder gpu): every row of every case must come back from
zlib.decompress(stream, -15) as it went in, with zlib's CRC-32, inside wc_deflate_bound; result-like rows must stay
within 1 % of zlib's own Z_RLE level-1 size; the assembled members must be the host writer's bytes; and the files written
through the GPU encoder must load identical to the host writer's."""
import heapq
import struct
import zipfile
import zlib

import numpy as np
import pytest

from wisecondor_amd import _lib
from wisecondor_amd import ingest
from wisecondor_amd import wisetools as wt

pytestmark = pytest.mark.gpu


def _B():
    return int(_lib.load().wc_deflate_block_bytes())


def _deflate(rows, src_pad=0, out_extra=0, dev=False):
    """rows: uint8 [n, L].  The streams of wc_deflate_rows (dev: wc_deflate_rows_dev on tensors) as a list of bytes, the
    CRCs, and the lengths; rows src_pad bytes further apart than they are long, output rows out_extra bytes above the
    bound.  The bytes behind every stream must be left alone."""
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    n, length = rows.shape
    lib = _lib.load()
    bound = int(lib.wc_deflate_bound(length))
    held = np.full((n, length + src_pad), 0x5A, dtype=np.uint8)
    held[:, :length] = rows
    stride = bound + out_extra
    if dev:
        import torch
        src = torch.from_numpy(held).cuda()
        streams, lengths, crcs = wt.deflateRows(src[:, :length], out_stride=stride)
        torch.cuda.synchronize()
        out = streams.cpu().numpy()
        lengths = lengths.cpu().numpy()
        crcs = crcs.cpu().numpy().view(np.uint32)
    else:
        out, lengths, crcs = wt.deflateRows(held[:, :length], out_stride=stride)
        assert not out[np.arange(stride)[None, :] >= lengths[:, None]].any()      # untouched behind the streams
    assert out.shape == (n, stride)
    return [out[i, :int(lengths[i])].tobytes() for i in range(n)], crcs, lengths


def _verify(rows, streams, crcs, lengths):
    bound = int(_lib.load().wc_deflate_bound(rows.shape[1]))
    for i, row in enumerate(rows):
        data = row.tobytes()
        assert zlib.decompress(streams[i], -15) == data, i
        assert int(crcs[i]) == zlib.crc32(data), i
        assert 0 < int(lengths[i]) <= bound, i


def _check(rows, **how):
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    got = _deflate(rows, **how)
    _verify(rows, *got)
    return got


def _distinct(n, seed=0, top=200):
    """n bytes below `top` without two equal neighbours."""
    rng = np.random.RandomState(seed)
    out = rng.randint(0, top, size=n).astype(np.uint8)
    for i in range(1, n):
        if out[i] == out[i - 1]:
            out[i] = (out[i] + 1) % top
    return out


def _zlib_rle(data):
    co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_RLE)
    return co.compress(data) + co.flush()


def _tree_depth(freq):
    heap = [(int(f), 0) for f in freq if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, da = heapq.heappop(heap)
        b, db = heapq.heappop(heap)
        heapq.heappush(heap, (a + b, max(da, db) + 1))
    return heap[0][1]


def test_row_lengths():
    B = _B()
    rng = np.random.RandomState(1)
    for length in (0, 1, 2, 3, B - 1, B, B + 1, 2 * B + 1):
        rows = np.stack([_distinct(length, 3, 16),                  # few symbols: coded
                         np.full(length, 7, dtype=np.uint8),            # one run
                         rng.randint(0, 256, size=length).astype(np.uint8)])
        _check(rows)


def test_runs_alone_in_a_row_of_distinct_bytes():
    runs = (2, 3, 4, 257, 258, 259, 260, 261, 516, 517, 518, 519)
    rows = np.stack([_distinct(700, 5, 64)] * len(runs))        # (coded blocks: 64 symbols)
    for i, run in enumerate(runs):
        rows[i, 50:50 + run] = 255
    streams, _, lengths = _check(rows)
    # a run is a literal and matches: 258 + 1 equal bytes cost far less than 259 literals
    assert lengths[5] < lengths[0]


def test_runs_at_block_cuts():
    B = _B()
    rows = np.stack([_distinct(2 * B + 100, 6, 32)] * 4)
    rows[0, B - 1:B + 9] = 255              # starts one byte before the cut
    rows[1, B - 8:B + 1] = 255              # ends one byte after it
    rows[2, B - 300:B + 300] = 255          # full matches on both sides
    rows[3, B:2 * B] = 255                  # a block that is one run
    _check(rows)


def test_degenerate_codes():
    B = _B()
    equal = np.full((1, B + 5), 0, dtype=np.uint8)
    streams, _, lengths = _check(equal)
    assert lengths[0] < 200
    # all 256 values, no run (no distance code is used), skewed enough that the block is coded, not stored
    every = np.concatenate([np.arange(256, dtype=np.uint8), _distinct(6000, 9, 4)])[None, :]
    assert not np.any(every[0, 1:] == every[0, :-1])
    streams, _, lengths = _check(np.concatenate([every, every[:, ::-1]]))
    assert np.all(lengths < 6256 // 2)
    two = (np.arange(3000) % 2).astype(np.uint8)[None, :] * 9
    streams, _, lengths = _check(two)
    assert lengths[0] < 3000 * 2 // 8 + 64  # three symbols with the end of block: at most two bits per byte, and a header


def test_length_limits():
    B = _B()
    fib = [1, 2]        # (the end-of-block symbol, once per block, is the sequence's first 1)
    while sum(fib) + fib[-1] + fib[-2] <= B:
        fib.append(fib[-1] + fib[-2])
    counts = sorted(fib + [B - sum(fib)], reverse=True)
    assert max(counts) <= B // 2
    seq = np.repeat(np.arange(len(counts), dtype=np.uint8) * 3, counts)       # most frequent first
    row = np.empty(B, dtype=np.uint8)
    row[0::2] = seq[:B // 2]
    row[1::2] = seq[B // 2:]
    assert not np.any(row[1:] == row[:-1])                                  # no run: every byte is a literal
    freq = np.bincount(row, minlength=256).tolist() + [1]                   # ... and the end-of-block symbol
    assert _tree_depth(freq) > 15
    streams, _, lengths = _check(np.stack([row, row[::-1]]))
    assert lengths[0] < B // 2


def test_stored_fallback():
    B = _B()
    rng = np.random.RandomState(2)
    for length in (B, 3 * B + 7):
        rows = rng.randint(0, 256, size=(2, length)).astype(np.uint8)
        _, _, lengths = _check(rows)
        assert np.all(lengths >= length)        # (and <= the bound: _verify)
        assert np.all(lengths <= length + 5 * -(-length // B))


def _result_rows(n_bins, seed):
    """The estimate's rows: float64 noise as z and as ratio - 1, 3 % of the bins zeroed singly and 12 runs of 5 .. 200."""
    rng = np.random.RandomState(seed)
    z = rng.standard_normal(n_bins)
    mask = np.ones(n_bins)
    mask[rng.uniform(size=n_bins) < 0.03] = 0.0
    for _ in range(12):
        at = int(rng.randint(0, n_bins - 200))
        mask[at:at + int(rng.randint(5, 201))] = 0.0
    return np.stack([z * mask, (1.0 + 0.03 * z) * mask - mask])


@pytest.mark.parametrize("n_bins", [11500, 57500])
def test_result_like_rows_stay_within_one_percent_of_zlib(n_bins):
    rows = _result_rows(n_bins, 2024).view(np.uint8)
    assert rows.shape == (2, 8 * n_bins)
    streams, _, lengths = _check(rows)
    for i in range(2):
        want = len(_zlib_rle(rows[i].tobytes()))
        print("n_bins %d row %d: %d bytes, zlib Z_RLE level 1 %d, ratio %.4f" % (n_bins, i, lengths[i], want, lengths[i] / want))
        assert lengths[i] <= 1.01 * want, (n_bins, i, int(lengths[i]), want)


def test_layout_and_determinism():
    B = _B()
    rng = np.random.RandomState(3)
    long_rows = np.concatenate([_result_rows(2 * B // 8 + 40, 7).view(np.uint8),
                                (rng.randint(0, 4, size=(1, 2 * B + 320)) * 60).astype(np.uint8)])
    first = _check(long_rows)
    for n_rows in (1, 3, 130):
        rows = (rng.randint(0, 6, size=(n_rows, 1000)) * (rng.uniform(size=(n_rows, 1000)) < 0.5)).astype(np.uint8)
        plain = _check(rows)
        for how in (dict(src_pad=37), dict(out_extra=13), dict(src_pad=3, out_extra=13, dev=True), dict(dev=True)):
            other = _check(rows, **how)
            assert other[0] == plain[0] and np.array_equal(other[1], plain[1])
    again = _check(long_rows)                   # after calls with shorter rows: nothing stale
    assert again[0] == first[0] and np.array_equal(again[1], first[1])
    assert _check(long_rows, dev=True)[0] == first[0]


def test_stream_through_the_projects_inflater():
    B = _B()
    rng = np.random.RandomState(4)
    row = np.concatenate([_distinct(B, 8, 16), rng.randint(0, 256, size=B).astype(np.uint8),
                          np.full(300, 9, dtype=np.uint8)])[None, :]     # a coded, a stored and a coded final block
    streams, crcs, _ = _check(row)
    data = row[0].tobytes()
    assert len(data) <= 65280 and len(streams[0]) + 26 <= 65536
    block = (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(streams[0]) + 25) + streams[0]
             + struct.pack("<II", int(crcs[0]), len(data)))
    empty = zlib.compressobj(6, zlib.DEFLATED, -15)
    empty = empty.compress(b"") + empty.flush()
    block += (struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(empty) + 25) + empty
              + struct.pack("<II", 0, 0))                               # the end-of-file block
    src = np.frombuffer(block, dtype=np.uint8).copy()
    out = np.zeros(len(data) + 8, dtype=np.uint8)
    n = np.zeros(1, dtype=np.int64)
    _lib.check(_lib.load().wc_bgzf_inflate(_lib.context(0), _lib.ptr(src), len(src), _lib.ptr(out), len(data), _lib.ptr(n)))
    assert int(n[0]) == len(data) and out[:len(data)].tobytes() == data


def _batch(sizes, n, seed):
    rng = np.random.RandomState(seed)
    n_total = int(np.sum(sizes))
    z = rng.standard_normal((n, n_total))
    z[:, ::7] = 0.0
    z[1, 100:400] = 0.0
    z[0, 3] = -0.0
    z[0, 5] = np.nan
    r = rng.standard_normal((n, n_total)) * 0.03
    r[z == 0.0] = 0.0
    cwz = rng.standard_normal((n, 22))
    calls = rng.standard_normal((n, 8, 5))
    n_calls = np.array(([3, 0, 8, 1, 2] * n)[:n], dtype=np.int32)
    asdef = rng.uniform(0.9, 1.1, size=n)
    return z, r, cwz, calls, n_calls, asdef


def _per_file(tmp_path, n, tag):
    import argparse
    return [argparse.Namespace(infile="in_%d.npz" % i, outfile="o_%d.npz" % i, minrefbins=25) for i in range(n)], \
        [str(tmp_path / ("%s_%d.npz" % (tag, i))) for i in range(n)]


def _same_files(path_a, path_b, skip=()):
    a = np.load(path_a, allow_pickle=True)
    b = np.load(path_b, allow_pickle=True)
    assert a.files == b.files
    for key in a.files:
        if key in skip:
            continue
        x, y = a[key], b[key]
        assert x.dtype == y.dtype and x.shape == y.shape, key
        if x.dtype == object and x.shape == ():
            assert x.item() == y.item(), key
        elif x.dtype == object:
            assert len(x) == len(y) and all(p.dtype == q.dtype and p.shape == q.shape and p.tobytes() == q.tobytes()
                                            for p, q in zip(x, y)), key
        else:
            assert x.tobytes() == y.tobytes(), key
    with zipfile.ZipFile(path_b) as zf:
        assert zf.testzip() is None
    return a, b


def test_member_image_and_written_files(tmp_path, golden):
    import torch
    sizes = [int(v) for v in golden("cfg1_pipeline.npz")["ref_chromosome_sizes"]]
    holed = list(sizes)
    holed[6] = 0
    for tag, chrom_sizes in (("full", sizes), ("holed", holed)):
        z, r, cwz, calls, n_calls, asdef = _batch(chrom_sizes, 3, 9)
        per_file, host = _per_file(tmp_path, 3, tag + "_host")
        _, gpu = _per_file(tmp_path, 3, tag + "_gpu")
        runtime = {"version": "v", "datetime": "d", "hostname": "h", "username": "u"}
        ingest.write_results(host, per_file, runtime, 1000000.0, 5.5, chrom_sizes, z, r, cwz, calls, n_calls, asdef)
        members = wt.ResultMembers(chrom_sizes, "cuda:0")
        image = members.image(torch.from_numpy(z).cuda()).cpu().numpy()
        for i in range(3):
            with zipfile.ZipFile(host[i]) as zf:
                assert image[i].tobytes() == zf.read("results_z.npy"), (tag, i)
        # the writer: device tensors in, the same files out (compared as np.load gives them: the floats' bits,
        # dtypes, shapes, the empty call list of the second sample)
        ingest.write_results(gpu, per_file, runtime, 1000000.0, 5.5, chrom_sizes, torch.from_numpy(z).cuda(),
                             torch.from_numpy(r).cuda(), torch.from_numpy(cwz).cuda(), torch.from_numpy(calls).cuda(),
                             torch.from_numpy(n_calls).cuda(), torch.from_numpy(asdef).cuda(), encoder="gpu")
        for i in range(3):
            a, b = _same_files(host[i], gpu[i])
            assert b["results_calls"].shape == ((n_calls[i], 5) if n_calls[i] else (0,))
            assert [len(v) for v in b["results_z"]] == chrom_sizes
            with zipfile.ZipFile(gpu[i]) as zf:
                assert zf.getinfo("results_z.npy").compress_type == zipfile.ZIP_DEFLATED
                assert zf.getinfo("results_r.npy").compress_size < zf.getinfo("results_r.npy").file_size


def test_testbatch_with_the_gpu_encoder(tmp_path, golden):
    from wisecondor_amd import wisecondor as cli
    g = golden("cfg1_pipeline.npz")
    lengths = g["sample_chrom_lengths"]
    keys = [str(c) for c in range(1, 23)] + ["X", "Y"]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    refpath = str(tmp_path / "reference.npz")
    np.savez_compressed(refpath, arguments={}, runtime={}, binsize=float(g["ref_binsize"]),
                        indexes=g["ref_indexes"], distances=g["ref_distances"],
                        chromosome_sizes=g["ref_chromosome_sizes"], mask=g["ref_mask"],
                        masked_sizes=g["ref_masked_sizes"], pca_components=g["ref_pca_components"],
                        pca_mean=g["ref_pca_mean"])
    rows = [g["t_%s_sample" % n] for n in ("mild18", "gain5_gap", "loss2", "normal")] + [g["ref_samples"][0]]
    paths = []
    for i, flat in enumerate(rows):
        p = str(tmp_path / ("s_%d.npz" % i))
        sample = {k: np.asarray(flat[offs[j]:offs[j + 1]], dtype=np.int32) for j, k in enumerate(keys)}
        np.savez_compressed(p, arguments={"binsize": float(g["binsize"])}, runtime={}, sample=sample, quality={})
        paths.append(p)
    cli.main(["testbatch"] + paths + [str(tmp_path / "host"), refpath, "-batch", "2"])
    cli.main(["testbatch"] + paths + [str(tmp_path / "gpu"), refpath, "-batch", "2", "-encoder", "gpu"])   # batches of 2, 2, 1
    for i in range(5):
        a, b = _same_files(str(tmp_path / "host" / ("s_%d_test.npz" % i)), str(tmp_path / "gpu" / ("s_%d_test.npz" % i)),
                           skip=("arguments", "runtime"))
        args_a, args_b = a["arguments"].item(), b["arguments"].item()
        assert "encoder" not in args_a and args_b["encoder"] == "gpu"
        assert args_b["outfile"].endswith("s_%d_test.npz" % i)
        assert {k: v for k, v in args_b.items() if k not in ("encoder", "outdir", "outfile")} == \
            {k: v for k, v in args_a.items() if k not in ("outdir", "outfile")}


def _text_like(n, seed):
    """n bytes of result-like text: the repr of float64 noise between commas, a fifth of the values 0.0."""
    rng = np.random.RandomState(seed)
    values = rng.standard_normal(n // 4 + 2) * (rng.uniform(size=n // 4 + 2) > 0.2)
    return np.frombuffer(",".join(repr(float(v)) for v in values).encode("ascii")[:n], dtype=np.uint8)


def _runs_over_cuts(n, B):
    """n distinct bytes with a run of 255 across every block cut (and up to the end, where the cut is the row's last byte)."""
    row = _distinct(n, 11, 64)
    for cut in range(B, n + 1, B):
        row[cut - 300:cut + 300] = 255
    return row


def test_rows_of_unequal_lengths_in_one_call():
    """wc_deflate_rows_len_dev: rows of every length regime, of text, of noise (stored blocks) and with runs over the block
    cuts, in ONE call from a source 3 bytes past a 16-byte boundary (export_json_batch's offset: the block coder's
    unaligned load), max_row_bytes the longest, so that short rows leave idle workgroups.  Every row's stream, length
    and CRC are those of wc_deflate_rows_dev on that row alone; a length out of range gives -1 and touches nothing."""
    import torch
    lib = _lib.load()
    ctx = _lib.context(0)
    B = _B()
    lengths = [0, 1, 63, 64, B - 1, B, B + 1, 2 * B, 2 * B + 5, 3 * B + 7]
    rng = np.random.RandomState(5)
    datas = []
    for length in lengths:
        datas += [_text_like(length, length), rng.randint(0, 256, size=length).astype(np.uint8), _runs_over_cuts(length, B)]
    n, most, fill = len(datas), max(lengths), 0xA5
    src_stride = (most + 3 + 15) // 16 * 16 + 16
    out_stride = int(lib.wc_deflate_bound(most)) + 13
    held = np.full(16 + n * src_stride, 0x5A, dtype=np.uint8)
    for i, data in enumerate(datas):
        held[3 + i * src_stride:3 + i * src_stride + len(data)] = data
    src = torch.from_numpy(held).cuda()
    assert src.data_ptr() % 16 == 0
    base = src.data_ptr() + 3
    stream = torch.cuda.current_stream().cuda_stream

    def run(row_len):
        out = torch.full((n, out_stride), fill, dtype=torch.uint8, device="cuda")
        out_len = torch.full((n,), -7, dtype=torch.int64, device="cuda")
        crc = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_len = torch.tensor(row_len, dtype=torch.int64, device="cuda")
        _lib.check(lib.wc_deflate_rows_len_dev(ctx, stream, base, n, d_len.data_ptr(), most, src_stride, out.data_ptr(), out_stride,
                                               out_len.data_ptr(), crc.data_ptr()))
        torch.cuda.synchronize()
        return out.cpu().numpy(), out_len.cpu().numpy(), crc.cpu().numpy().view(np.uint32)

    # the reference: every row alone through the fixed-length entry, from where it lies
    alone = []
    for i, data in enumerate(datas):
        one = torch.full((out_stride,), fill, dtype=torch.uint8, device="cuda")
        one_len = torch.zeros(1, dtype=torch.int64, device="cuda")
        one_crc = torch.zeros(1, dtype=torch.int32, device="cuda")
        _lib.check(lib.wc_deflate_rows_dev(ctx, stream, base + i * src_stride, 1, len(data), len(data), one.data_ptr(), out_stride,
                                           one_len.data_ptr(), one_crc.data_ptr()))
        alone.append((one.cpu().numpy(), int(one_len[0]), int(one_crc[0]) & 0xffffffff))

    def check_row(i, out, out_len, crc):
        data = datas[i].tobytes()
        want, want_len, want_crc = alone[i]
        assert int(out_len[i]) == want_len and 0 < want_len <= out_stride, (i, int(out_len[i]), want_len)
        assert out[i, :want_len].tobytes() == want[:want_len].tobytes(), i
        assert int(crc[i]) == want_crc == zlib.crc32(data), i
        assert zlib.decompress(out[i, :want_len].tobytes(), -15) == data, i
        assert np.all(out[i, want_len:] == fill), i

    row_len = [len(d) for d in datas]
    got = run(row_len)
    for i in range(n):
        check_row(i, *got)
    stored = [i for i in range(n) if i % 3 == 1 and len(datas[i]) >= 64]
    assert all(got[1][i] >= len(datas[i]) for i in stored)                 # noise takes the stored fallback
    bad = {13: -1, 22: most + 1}
    got = run([bad.get(i, v) for i, v in enumerate(row_len)])
    for i in range(n):
        if i in bad:
            assert int(got[1][i]) == -1 and np.all(got[0][i] == fill), i
        else:
            check_row(i, *got)
