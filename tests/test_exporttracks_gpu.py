"""exporttracks on the GPU: every case's text (tests/tracks_cases.py) against the restatement (tests/tracks_restated.py)
byte for byte, the refusals, the BGZF rows against zlib, gzip, the project's own inflater and the tested deflate entry,
export_tracks_batch and the command line.

The kernels' sizes: a tile is 256 bins (csrc/tracks.hip); a BGZF block is B = wc_deflate_block_bytes() = 16 384 input
bytes (csrc/deflate.hip)."""
import gzip
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import json_cases  # noqa: E402
import tracks_cases as tc  # noqa: E402
import tracks_restated as tr  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x55


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


def rows_host(sizes, rows, binsize, prefix="chr", clip=None, nozero=False, stride=None, text_stride=None, n_rows=None, flags=None):
    """wc_bedgraph_rows on rows [n, stride]: (rc, the texts, the whole text buffer, text_len, dropped)."""
    from wisecondor_amd import _lib
    lib = _lib.load()
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    raw = prefix.encode("ascii")
    clip = None if clip is None else np.ascontiguousarray(clip, dtype=np.int64)
    bound = int(lib.wc_bedgraph_row_bound(_lib.ptr(sizes), len(sizes), binsize, min(len(raw), 16)))
    room = max(bound, 0) + 5                                # (a text_stride beyond it goes with calls that are refused)
    text_stride = room if text_stride is None else text_stride
    n = rows.shape[0]
    text = np.full((n, room), FILL, dtype=np.uint8)
    lens = np.full(n, -7, dtype=np.int64)
    dropped = np.full(n, -7, dtype=np.int64)
    rc = lib.wc_bedgraph_rows(_lib.context(0), _lib.ptr(rows), rows.shape[1] if stride is None else stride, n if n_rows is None else n_rows,
                              _lib.ptr(sizes), len(sizes), binsize, _lib.ptr(clip), raw, len(raw), int(nozero) if flags is None else flags,
                              _lib.ptr(text), text_stride, _lib.ptr(lens), _lib.ptr(dropped), None)
    texts = [text[i, :max(int(lens[i]), 0)].tobytes() for i in range(n)] if rc == 0 else None
    return rc, texts, text, lens, dropped


def check_rows(sizes, rows, binsize, prefix="chr", clip=None, nozero=False):
    total = int(sum(sizes))
    rc, texts, text, lens, dropped = rows_host(sizes, rows, binsize, prefix, clip, nozero)
    assert rc == 0
    for i in range(rows.shape[0]):
        want, want_dropped = tr.track_text(rows[i, :total], sizes, binsize, prefix, clip, nozero)
        if texts[i] != want:
            at = next((k for k in range(min(len(want), len(texts[i]))) if texts[i][k] != want[k]), min(len(want), len(texts[i])))
            raise AssertionError("row %d (%d bytes, the restatement has %d) differs at byte %d: %r, the restatement has %r"
                                 % (i, lens[i], len(want), at, texts[i][max(0, at - 40):at + 40], want[max(0, at - 40):at + 40]))
        assert lens[i] == len(want) and dropped[i] == want_dropped, (i, lens[i], len(want), dropped[i], want_dropped)
        assert np.all(text[i, lens[i]:] == FILL)            # the host form writes text_len bytes of every row
    return texts


@pytest.mark.parametrize("name", [c["name"] for c in tc.cases()])
def test_every_case_equals_the_restatement(name):
    case = tc.by_name(name)
    texts = check_rows(case["sizes"], case["rows"], case["binsize"], case["prefix"], case["clip"], case["nozero"])
    if name.startswith("everything_left_out"):
        assert texts == [b""] * len(texts)


@pytest.mark.parametrize("n_rows", [1, 3, 130])
def test_rows_with_padded_strides(n_rows):
    rows = tc.result_like_rows(n_rows)
    plain = check_rows(tc.SIZES, rows, 250000)
    padded = tc.padded(rows, rows.shape[1] + 37)            # the padding holds 7e77, which must not show
    assert check_rows(tc.SIZES, padded, 250000) == plain
    assert all(b"7e+77" not in t for t in plain)
    check_rows(tc.SIZES, padded, 250000, nozero=True)


def test_the_same_bytes_twice_and_after_a_call_with_longer_rows():
    small = tc.by_name("boundary_on_a_tile_edge")
    first = check_rows(small["sizes"], small["rows"], small["binsize"])
    assert check_rows(small["sizes"], small["rows"], small["binsize"]) == first
    big = tc.by_name("run_across_three_tiles")
    check_rows(big["sizes"], np.repeat(big["rows"], 6, axis=0), big["binsize"])
    assert check_rows(small["sizes"], small["rows"], small["binsize"]) == first


def test_limits_and_refusals_leave_the_outputs_untouched():
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    rows = np.ones((2, 8))

    def refused(code, sizes=(5, 0, 3), binsize=1000, **more):
        rc, _, text, lens, dropped = rows_host(list(sizes), rows, binsize, **more)
        assert rc == code, (rc, lib.wc_last_error())
        assert np.all(text == FILL) and np.all(lens == -7) and np.all(dropped == -7)

    refused(_lib.E_LIMIT, sizes=[3], binsize=333333333333334)          # a coordinate of 16 digits
    refused(_lib.E_LIMIT, sizes=[1], binsize=10 ** 15)
    assert rows_host([3], rows, 333333333333333)[0] == 0                # 999 999 999 999 999 is written
    refused(_lib.E_ARG, prefix="x" * 17)
    refused(_lib.E_ARG, prefix="a\tb")
    refused(_lib.E_ARG, prefix="a\nb")
    refused(_lib.E_ARG, binsize=0)
    refused(_lib.E_ARG, sizes=[5, -1, 3])
    refused(_lib.E_ARG, n_rows=-1)
    refused(_lib.E_ARG, stride=7)
    refused(_lib.E_ARG, flags=2)
    refused(_lib.E_ARG, clip=[4000, 1, 3000])                           # chromosome 1's last bin starts at 4000
    refused(_lib.E_LIMIT, n_rows=65536)
    refused(_lib.E_LIMIT, sizes=[1] * 65, stride=65)
    refused(_lib.E_LIMIT, sizes=[1 << 30, 1 << 30], binsize=1, stride=1 << 40, text_stride=1 << 50)
    bound = int(lib.wc_bedgraph_row_bound(_lib.ptr(np.array([5, 0, 3], dtype=np.int64)), 3, 1000, 3))
    refused(_lib.E_ARG, text_stride=bound - 1)
    assert rows_host([5, 0, 3], rows, 1000, text_stride=bound)[0] == 0
    # the device form also wants rows that start on multiples of 16
    s = np.array([5, 0, 3], dtype=np.int64)
    d_rows = torch.ones((2, 8), dtype=torch.float64, device="cuda")
    stride = (bound + 15) // 16 * 16
    text = torch.full((2 * stride + 64,), FILL, dtype=torch.uint8, device="cuda")
    counts = torch.full((2, 2), -7, dtype=torch.int64, device="cuda")
    for shift, step in ((8, stride), (0, stride + 8), (0, stride - 16)):
        rc = lib.wc_bedgraph_rows_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_rows.data_ptr(), 8, 2, _lib.ptr(s), 3, 1000,
                                      None, b"chr", 3, 0, text.data_ptr() + shift, step, counts[0].data_ptr(), counts[1].data_ptr())
        assert rc == _lib.E_ARG, (rc, lib.wc_last_error())
    torch.cuda.synchronize()
    assert bool((text == FILL).all()) and bool((counts == -7).all())


def test_device_form_gives_the_host_forms_bytes_and_leaves_the_rest_alone(wt):
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    sizes = np.array(tc.SIZES, dtype=np.int64)
    rows = tc.padded(tc.result_like_rows(3), int(sizes.sum()) + 3)
    clip = np.array([max(1, n * 250000 - 1000) for n in tc.SIZES], dtype=np.int64)
    for nozero in (False, True):
        want, want_dropped = wt.bedgraphRows(rows, sizes, 250000, clip=clip, nozero=nozero, row_stride=rows.shape[1])
        for i in range(3):
            assert (want[i], want_dropped[i]) == tr.track_text(rows[i], tc.SIZES, 250000, clip=clip, nozero=nozero)
        stride = (wt.bedgraphRowBound(sizes, 250000, 3) + 15) // 16 * 16 + 32
        d_rows = torch.from_numpy(rows).cuda()
        text = torch.full((3, stride), FILL, dtype=torch.uint8, device="cuda")
        counts = torch.full((2, 3), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.wc_bedgraph_rows_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_rows.data_ptr(), rows.shape[1], 3,
                                            _lib.ptr(sizes), len(sizes), 250000, _lib.ptr(clip), b"chr", 3, int(nozero), text.data_ptr(), stride,
                                            counts[0].data_ptr(), counts[1].data_ptr()))
        got, got_counts = text.cpu().numpy(), counts.cpu().numpy()
        assert got_counts[1].tolist() == want_dropped
        for i in range(3):
            assert got[i, :got_counts[0][i]].tobytes() == want[i]
            assert np.all(got[i, got_counts[0][i]:] == FILL)        # the header: bytes behind text_len[i] are not written


# ---------------------------------------------------------------------------------------------------- BGZF ----
def _text_like(n, seed):
    rng = np.random.RandomState(seed)
    lines = b"".join(b"chr%d\t%d\t%d\t%r\n" % (1 + k % 22, k * 50000, (k + 1) * 50000, float(rng.standard_normal())) for k in range(n // 30 + 2))
    return lines[:n]


def bgzf_rows(datas, pad=19, device=False):
    """wc_bgzf_rows (or the _dev form on device tensors) on the byte strings `datas` in one call: the rows' bytes."""
    from wisecondor_amd import _lib
    lib = _lib.load()
    longest = max(len(d) for d in datas)
    stride = longest + pad
    src = np.full((len(datas), stride), 0xEE, dtype=np.uint8)
    for i, d in enumerate(datas):
        src[i, :len(d)] = np.frombuffer(d, dtype=np.uint8)
    lens = np.array([len(d) for d in datas], dtype=np.int64)
    out_stride = int(lib.wc_bgzf_bound(longest)) + 7
    if device:
        import torch
        d_src, d_lens = torch.from_numpy(src).cuda(), torch.from_numpy(lens).cuda()
        d_out = torch.full((len(datas), out_stride), FILL, dtype=torch.uint8, device="cuda")
        d_n = torch.full((len(datas),), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.wc_bgzf_rows_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_src.data_ptr(), len(datas), d_lens.data_ptr(),
                                        longest, stride, d_out.data_ptr(), out_stride, d_n.data_ptr()))
        out, n = d_out.cpu().numpy(), d_n.cpu().numpy()
    else:
        out = np.full((len(datas), out_stride), FILL, dtype=np.uint8)
        n = np.full(len(datas), -7, dtype=np.int64)
        _lib.check(lib.wc_bgzf_rows(_lib.context(0), _lib.ptr(src), len(datas), _lib.ptr(lens), longest, stride, _lib.ptr(out), out_stride,
                                    _lib.ptr(n)))
    for i, d in enumerate(datas):
        assert 28 <= n[i] <= lib.wc_bgzf_bound(len(d)), (i, n[i], len(d))
        assert np.all(out[i, n[i]:] == FILL)                # bytes behind out_len[i] are not written
    return [out[i, :n[i]].tobytes() for i in range(len(datas))]


def inflate_own(blob, cap):
    from wisecondor_amd import _lib
    src = np.frombuffer(blob, dtype=np.uint8).copy()
    out = np.zeros(cap + 8, dtype=np.uint8)
    n = np.zeros(1, dtype=np.int64)
    _lib.check(_lib.load().wc_bgzf_inflate(_lib.context(0), _lib.ptr(src), len(src), _lib.ptr(out), cap, _lib.ptr(n)))
    return out[:int(n[0])].tobytes()


def check_bgzf(datas, files, B):
    for data, blob in zip(datas, files):
        blocks = tr.bgzf_blocks(blob)                       # the walk by BSIZE ends exactly at the last byte
        assert blob[-28:] == tr.BGZF_EOF and blocks[-1] == (b"\x03\x00", 0, 0)
        assert len(blocks) == (len(data) + B - 1) // B + 1
        for k, (payload, crc, isize) in enumerate(blocks[:-1]):
            piece = data[k * B:(k + 1) * B]
            assert zlib.decompress(payload, -15) == piece, k
            assert crc == zlib.crc32(piece) and isize == len(piece), k
        assert gzip.decompress(blob) == data
        assert inflate_own(blob, len(data)) == data


def test_bgzf_rows_of_every_length_in_one_call(wt):
    from wisecondor_amd import _lib
    B = _lib.load().wc_deflate_block_bytes()
    lengths = [0, 1, 2, B - 1, B, B + 1, 2 * B + 1]
    datas = [_text_like(n, 30 + i) for i, n in enumerate(lengths)]
    assert [len(d) for d in datas] == lengths
    host = bgzf_rows(datas)
    check_bgzf(datas, host, B)
    assert host[0] == tr.BGZF_EOF
    assert bgzf_rows(datas, device=True) == host
    # after a call with longer rows, and the rows in another order: the same files
    longer = [_text_like(3 * B + 5, 50), _text_like(5, 51)]
    check_bgzf(longer, bgzf_rows(longer, pad=3, device=True), B)
    assert bgzf_rows(datas[::-1], pad=64) == host[::-1]
    # the raw deflate bytes of a block are what the tested entry gives for that block's input alone (a row's last block)
    pieces = {}
    for data, blob in zip(datas, host):
        for k, (payload, _, _) in enumerate(tr.bgzf_blocks(blob)[:-1]):
            pieces.setdefault(len(data[k * B:(k + 1) * B]), []).append((data[k * B:(k + 1) * B], payload))
    assert sorted(pieces) == [1, 2, B - 1, B]
    for n, pairs in pieces.items():
        rows = np.stack([np.frombuffer(piece, dtype=np.uint8) for piece, _ in pairs])
        streams, lens, crcs = wt.deflateRows(rows)
        for i, (piece, payload) in enumerate(pairs):
            assert streams[i, :lens[i]].tobytes() == payload, (n, i)
            assert crcs[i] == zlib.crc32(piece)


def test_bgzf_stored_fallback_and_compression():
    from wisecondor_amd import _lib
    B = _lib.load().wc_deflate_block_bytes()
    rng = np.random.RandomState(8)
    noise = [bytes(rng.randint(0, 256, size=n).astype(np.uint8)) for n in (B + 77, 300)]
    line = b"chr7\t50000\t100000\t0.0\n"
    repeated = (line * (3 * B // len(line) + 1))[:2 * B + 100]
    datas = noise + [repeated, b"\x00" * (B + 1)]
    files = bgzf_rows(datas)
    check_bgzf(datas, files, B)
    for data, blob in zip(noise, files):
        for k, (payload, _, isize) in enumerate(tr.bgzf_blocks(blob)[:-1]):
            # incompressible: a stored block, final, its length and the length's complement in front of the bytes
            assert len(payload) == isize + 5 and payload[0] == 1 and payload[5:] == data[k * B:k * B + isize]
    assert len(files[2]) < len(repeated) and len(files[3]) < len(datas[3]) // 4
    # a length outside 0 .. max_row_bytes: the host form refuses it
    lib = _lib.load()
    src = np.zeros((2, 64), dtype=np.uint8)
    out = np.full((2, 200), FILL, dtype=np.uint8)
    n = np.full(2, -7, dtype=np.int64)
    for lens in ([5, 41], [-1, 5]):
        rc = lib.wc_bgzf_rows(_lib.context(0), _lib.ptr(src), 2, _lib.ptr(np.array(lens, dtype=np.int64)), 40, 64, _lib.ptr(out), 200, _lib.ptr(n))
        assert rc == _lib.E_ARG and np.all(out == FILL) and np.all(n == -7)
    rc = lib.wc_bgzf_rows(_lib.context(0), _lib.ptr(src), 2, _lib.ptr(np.array([5, 40], dtype=np.int64)), 40, 64, _lib.ptr(out),
                          lib.wc_bgzf_bound(40) - 1, _lib.ptr(n))
    assert rc == _lib.E_ARG and np.all(out == FILL)


def test_bgzf_dev_marks_a_row_whose_length_is_out_of_range():
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    src = torch.full((3, 64), 65, dtype=torch.uint8, device="cuda")
    lens = torch.tensor([41, 7, -1], dtype=torch.int64, device="cuda")
    out = torch.full((3, 128), FILL, dtype=torch.uint8, device="cuda")
    n = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    assert lib.wc_bgzf_bound(40) <= 128
    _lib.check(lib.wc_bgzf_rows_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, src.data_ptr(), 3, lens.data_ptr(), 40, 64,
                                    out.data_ptr(), 128, n.data_ptr()))
    got, got_n = out.cpu().numpy(), n.cpu().numpy()
    assert got_n[0] == -1 and got_n[2] == -1 and np.all(got[0] == FILL) and np.all(got[2] == FILL)
    assert gzip.decompress(got[1, :got_n[1]].tobytes()) == b"A" * 7


# ---------------------------------------------------------------------- the library call and the command line ----
def _write_results(tmp_path, seeds):
    from wisecondor_amd import wisecondor as cli
    paths, results = [], []
    for seed in seeds:
        res = json_cases.synthetic_result(seed, n_calls=seed % 4)
        res["results_z"] = [c.copy() for c in res["results_z"]]
        res["results_z"][12][100:400] = 0.0                 # a masked stretch across a tile edge
        res["results_r"] = [c.copy() for c in res["results_r"]]
        res["results_r"][13][:] = 0.0
        path = str(tmp_path / ("s%d_test.npz" % seed))
        cli.write_npz(path, arguments={"repeats": 5}, runtime={"host": "x"}, binsize=res["binsize"],
                      results_r=cli._as_object_array(res["results_r"]), results_z=cli._as_object_array(res["results_z"]),
                      results_cwz=res["results_cwz"], results_calls=res["results_calls"], threshold_z=res["threshold_z"],
                      asdef=res["asdef"], aasdef=res["aasdef"])
        paths.append(path)
        results.append(res)
    return paths, results


def _want(res, key, clip=None, nozero=False, prefix="chr"):
    row = np.concatenate(res["results_" + key])
    return tr.track_text(row, json_cases.SIZES, res["binsize"], prefix, clip, nozero)


def test_export_tracks_batch(wt):
    results = [json_cases.synthetic_result(20 + i, n_calls=i) for i in range(5)]
    details = {}
    files = wt.export_tracks_batch(results, details=details)
    assert len(files) == 5 and all(len(f) == 3 for f in files)
    for i, (res, (z, r, bed)) in enumerate(zip(results, files)):
        assert (z, details["dropped"][i][0]) == _want(res, "z") and (r, details["dropped"][i][1]) == _want(res, "r")
        assert bed == tr.calls_bed(np.asarray(res["results_calls"]).reshape(-1, 5), res["binsize"])
        assert details["text_bytes"][i] == (len(z), len(r))
    assert wt.export_tracks_batch(results) == files                      # the same bytes from a second call
    # split at two rows per GPU call and at a byte budget that holds one file: the same files
    assert wt.export_tracks_batch(results, max_rows=2) == files and wt.export_tracks_batch(results, max_bytes=1) == files
    # the host form gives the device form's bytes
    texts, _ = wt.bedgraphRows(np.stack([np.concatenate(res["results_z"]) for res in results]), json_cases.SIZES, 250000)
    assert texts == [f[0] for f in files]
    clip = [max(1, n * 250000 - 1000) for n in json_cases.SIZES]
    packed = wt.export_tracks_batch(results, only="r", gz=True, nozero=True, prefix="", chrom_lengths=clip, mineffect=4.0, max_rows=3)
    for res, (r, bed) in zip(results, packed):
        assert gzip.decompress(r) == _want(res, "r", clip, True, "")[0]
        tr.bgzf_blocks(r)
        assert bed == tr.calls_bed(np.asarray(res["results_calls"]).reshape(-1, 5), res["binsize"], "", clip, 4.0)
    assert wt.export_tracks_batch([]) == []
    with pytest.raises(ValueError):
        wt.export_tracks_batch(results, only="x")
    with pytest.raises(ValueError):
        wt.export_tracks_batch(results + [dict(results[0], binsize=50000)])


def test_exporttracks_command_line(tmp_path, capsys):
    """Five files in batches of two, one in the middle cannot be read; plain and -gz with -nozero, -only r, -chromsizes."""
    from wisecondor_amd import wisecondor as cli
    paths, results = _write_results(tmp_path, [1, 2, 3, 4])
    damaged = str(tmp_path / "damaged_test.npz")
    with open(damaged, "wb") as f:
        f.write(open(paths[0], "rb").read()[:200])
    given = [paths[0], paths[1], damaged, paths[2], paths[3]]
    plain = tmp_path / "plain"
    with pytest.raises(SystemExit) as stop:
        cli.main(["exporttracks"] + given + [str(plain), "-batch", "2"])
    assert stop.value.code == 1
    said = capsys.readouterr().out
    assert "damaged_test.npz skipped: cannot be read" in said and "4 result files as tracks" in said
    dropped = sum(_want(res, key)[1] for res in results for key in ("z", "r"))
    assert dropped > 0 and "(%d bins left out as not finite)" % dropped in said
    assert sorted(os.listdir(str(plain))) == sorted("s%d_test_%s" % (s, e) for s in (1, 2, 3, 4) for e in ("z.bedgraph", "r.bedgraph", "calls.bed"))
    for seed, res in zip((1, 2, 3, 4), results):
        for key in ("z", "r"):
            assert open(str(plain / ("s%d_test_%s.bedgraph" % (seed, key))), "rb").read() == _want(res, key)[0]
        assert open(str(plain / ("s%d_test_calls.bed" % seed)), "rb").read() == \
            tr.calls_bed(np.asarray(res["results_calls"]).reshape(-1, 5), res["binsize"])
    # -gz -nozero -only r -chromsizes against a plain run with the same options
    sizes = tmp_path / "genome.sizes"
    clip = [max(1, n * 250000 - 1000) for n in json_cases.SIZES]
    sizes.write_text("".join("chr%d\t%d\n" % (i + 1, n) for i, n in enumerate(clip)) + "chrX\t1000\n")
    options = ["-batch", "2", "-nozero", "-only", "r", "-chromsizes", str(sizes), "-mineffect", "4"]
    flat, packed = tmp_path / "flat", tmp_path / "packed"
    cli.main(["exporttracks"] + paths + [str(flat)] + options)
    cli.main(["exporttracks"] + paths + [str(packed), "-gz"] + options)
    assert "4 result files as tracks" in capsys.readouterr().out
    assert sorted(os.listdir(str(packed))) == sorted("s%d_test_%s" % (s, e) for s in (1, 2, 3, 4) for e in ("r.bedgraph.gz", "calls.bed"))
    for seed, res in zip((1, 2, 3, 4), results):
        text = open(str(flat / ("s%d_test_r.bedgraph" % seed)), "rb").read()
        assert text == _want(res, "r", clip, True)[0]
        with gzip.open(str(packed / ("s%d_test_r.bedgraph.gz" % seed)), "rb") as f:
            assert f.read() == text
        tr.bgzf_blocks(open(str(packed / ("s%d_test_r.bedgraph.gz" % seed)), "rb").read())
        bed = open(str(packed / ("s%d_test_calls.bed" % seed)), "rb").read()
        assert bed == open(str(flat / ("s%d_test_calls.bed" % seed)), "rb").read() == \
            tr.calls_bed(np.asarray(res["results_calls"]).reshape(-1, 5), res["binsize"], "chr", clip, 4.0)
    # a -chromsizes file that lacks a chromosome, or is too short for the bins: exit status 2
    for content, said in (("".join("chr%d\t%d\n" % (i + 1, n) for i, n in enumerate(clip[:-1])), "has no chromosome chr22"),
                          ("".join("chr%d\t%d\n" % (i + 1, 250000) for i in range(22)), "bases, the result files have")):
        sizes.write_text(content)
        with pytest.raises(SystemExit) as stop:
            cli.main(["exporttracks"] + paths + [str(tmp_path / "refused"), "-chromsizes", str(sizes)])
        assert stop.value.code == 2 and said in capsys.readouterr().out
        assert not os.path.isdir(str(tmp_path / "refused")) or not os.listdir(str(tmp_path / "refused"))


def test_a_file_whose_bin_size_is_no_positive_whole_number_is_skipped(tmp_path, capsys):
    from wisecondor_amd import wisecondor as cli
    paths, results = _write_results(tmp_path, [5, 6])
    res = results[1]
    for k, binsize in enumerate((250000.5, 0, -250000)):
        path = str(tmp_path / ("odd%d_test.npz" % k))
        cli.write_npz(path, arguments={}, runtime={}, binsize=binsize, results_r=cli._as_object_array(res["results_r"]),
                      results_z=cli._as_object_array(res["results_z"]), results_cwz=res["results_cwz"], results_calls=res["results_calls"],
                      threshold_z=res["threshold_z"], asdef=res["asdef"], aasdef=res["aasdef"])
        paths.append(path)
    with pytest.raises(SystemExit) as stop:
        cli.main(["exporttracks"] + paths + [str(tmp_path / "out"), "-only", "z"])
    assert stop.value.code == 1
    said = capsys.readouterr().out
    assert said.count("is not a positive whole number") == 3 and "2 result files as tracks" in said
    assert sorted(os.listdir(str(tmp_path / "out"))) == sorted("s%d_test_%s" % (s, e) for s in (5, 6) for e in ("z.bedgraph", "calls.bed"))
