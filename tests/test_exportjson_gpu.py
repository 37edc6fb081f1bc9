"""exportjson on the GPU: the device's digits against CPython and the host routine, the rows' text against the
restatement (tests/json_restated.py) byte for byte, the refusals, the command line and the gzip members.

The kernels' sizes (csrc/export.hip): a tile is JS_T = 256 values; k_js_scan sums 256 tiles per trip (65 536 values);
a tile's image leaves LDS in trips of 256 lines of 16 bytes (4 096 bytes; a tile of "0.0," fields is 1 024 bytes,
one of 24-byte values 6 400)."""
import gzip
import json
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import json_cases  # noqa: E402
import json_restated as jr  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 256
SCAN_TRIP = 256 * TILE
LONGEST = -1.2345678901234567e-308      # 24 bytes
FILL = 0x55


@pytest.fixture(scope="module")
def wt():
    from wisecondor_amd import wisetools
    return wisetools


def rows_host(sizes, rows, strict=False, stride=None, text_stride=None, times=None):
    """wc_json_rows on rows [n, stride]: (rc, the texts, the whole text buffer, text_len)."""
    from wisecondor_amd import _lib
    lib = _lib.load()
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    bound = int(lib.wc_json_row_bound(_lib.ptr(sizes), len(sizes)))
    text_stride = bound + 5 if text_stride is None else text_stride
    text = np.full((rows.shape[0], max(text_stride, 1)), FILL, dtype=np.uint8)
    lens = np.full(rows.shape[0], -7, dtype=np.int64)
    rc = lib.wc_json_rows(_lib.context(0), _lib.ptr(rows), rows.shape[1] if stride is None else stride, rows.shape[0], _lib.ptr(sizes),
                          len(sizes), int(strict), _lib.ptr(text), text_stride, _lib.ptr(lens), _lib.ptr(times))
    texts = [text[i, :max(int(lens[i]), 0)].tobytes() for i in range(rows.shape[0])] if rc == 0 else None
    return rc, texts, text, lens


def check_rows(sizes, rows, strict=False):
    total = int(sum(sizes))
    rc, texts, text, lens = rows_host(sizes, rows, strict)
    assert rc == 0
    for i in range(rows.shape[0]):
        want = jr.row_text(rows[i, :total], sizes, strict)
        assert lens[i] == len(want), (i, lens[i], len(want))
        if texts[i] != want:
            at = next(k for k in range(len(want)) if texts[i][k] != want[k])
            raise AssertionError("row %d differs at byte %d: %r, the restatement has %r" % (i, at, texts[i][max(0, at - 30):at + 30],
                                                                                          want[max(0, at - 30):at + 30]))
        assert np.all(text[i, lens[i]:] == FILL)            # the host form writes text_len bytes of every row
    return texts


@pytest.mark.parametrize("strict", [False, True])
def test_device_digits_equal_cpython_and_the_host_routine(strict):
    from wisecondor_amd import _lib
    lib = _lib.load()
    values = json_cases.digit_inputs()
    want = json_cases.digit_expected(strict)
    text = np.full((len(values), 24), FILL, dtype=np.uint8)
    lens = np.zeros(len(values), dtype=np.uint8)
    assert lib.wc_format_doubles(_lib.context(0), _lib.ptr(values), len(values), int(strict), _lib.ptr(text), _lib.ptr(lens)) == 0
    got = text.reshape(-1).view("S24")
    bad = np.nonzero(got != want)[0][:5]
    assert not len(bad), [(values[i].hex(), want[i], got[i]) for i in bad]
    host = np.full((len(values), 24), FILL, dtype=np.uint8)
    host_lens = np.zeros(len(values), dtype=np.uint8)
    assert lib.wc_format_doubles_host(_lib.ptr(values), len(values), int(strict), _lib.ptr(host), _lib.ptr(host_lens)) == 0
    assert np.array_equal(text, host) and np.array_equal(lens, host_lens)
    # a count that is no multiple of the tile, and one value
    for n in (1, TILE - 1, TILE + 1):
        part = np.ascontiguousarray(values[1000000:1000000 + n])
        t = np.full((n, 24), FILL, dtype=np.uint8)
        ln = np.zeros(n, dtype=np.uint8)
        assert lib.wc_format_doubles(_lib.context(0), _lib.ptr(part), n, int(strict), _lib.ptr(t), _lib.ptr(ln)) == 0
        assert np.array_equal(t, host[1000000:1000000 + n]) and np.array_equal(ln, host_lens[1000000:1000000 + n])


@pytest.mark.parametrize("n_rows", [1, 3, 130])
def test_rows_equal_the_restatement(n_rows):
    sizes = json_cases.SIZES
    arrays = [json_cases.synthetic_result(100 + i)["results_z" if i % 2 == 0 else "results_r"] for i in range(n_rows)]
    check_rows(sizes, json_cases.dense(arrays))
    padded = json_cases.dense(arrays[:3], stride=sum(sizes) + 37)      # the padding holds 7e77, which must not show
    texts = check_rows(sizes, padded)
    assert all(b"7e+77" not in t for t in texts)
    check_rows(sizes, padded, strict=True)


def test_rows_at_every_tile_and_trip_size():
    rng = np.random.RandomState(3)
    cases = [[], [0], [0, 0, 0], [1], [0, 1], [1, 0], [1, 0, 0, 1, 0]]
    for n in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1):
        cases += [[n], [0, n, 0], [n, 1], [1, n], [3, n, n]]
    for n in (SCAN_TRIP - 1, SCAN_TRIP, SCAN_TRIP + 1):
        cases += [[n], [TILE, 0, n - TILE]]
    for sizes in cases:
        total = sum(sizes)
        rows = np.round(rng.standard_normal((2, max(total, 1))) * 3.0, rng.randint(0, 17))
        rows[1] = rng.standard_normal(max(total, 1)) * 10.0 ** rng.randint(-30, 30, size=max(total, 1))
        texts = check_rows(sizes, rows)
        if total == 0:
            assert texts[0] == ("[" + ",".join("[]" for _ in sizes) + "]").encode()


def test_rows_of_extreme_fields(wt):
    sizes = [TILE + 44, 0, 3 * TILE + 1, 1]       # exactly one empty chromosome: the bound is reached
    total = sum(sizes)
    rows = np.zeros((4, total))
    rows[1] = LONGEST
    rows[2, 0::2] = LONGEST
    rows[3, 1::2] = LONGEST
    rows[3, 0::2] = float("nan")                # three bytes, as 0.0 is
    texts = check_rows(sizes, rows)
    assert set(texts[0]) == set(b"[],0.")
    assert len(texts[1]) == wt.jsonRowBound(sizes) == 25 * total + 2 * len(sizes) + 2
    assert len(json.dumps(LONGEST)) == 24 and len(json.dumps(0.0)) == 3
    strict = check_rows(sizes, rows, strict=True)
    assert b"null" in strict[3] and b"NaN" not in strict[3]
    # several empty chromosomes: the bound grows by one for each beyond the first, and is reached
    sizes = [0, 2, 0, 0, TILE, 0]
    rows = np.full((1, sum(sizes)), LONGEST)
    texts = check_rows(sizes, rows)
    assert len(texts[0]) == wt.jsonRowBound(sizes) == 25 * sum(sizes) + 2 * len(sizes) + 2 + 3


def test_the_same_bytes_twice_and_after_a_larger_job():
    sizes = json_cases.SIZES
    small = json_cases.dense([json_cases.synthetic_result(7)["results_z"]] * 2)
    first = check_rows(sizes, small)
    assert check_rows(sizes, small) == first
    big = np.random.RandomState(9).standard_normal((12, 3 * SCAN_TRIP // 4))
    check_rows([big.shape[1] - 5, 5], big)
    assert check_rows(sizes, small) == first


def test_device_form_gives_the_host_forms_bytes_and_leaves_the_rest_alone(wt):
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    sizes = np.array(json_cases.SIZES, dtype=np.int64)
    arrays = [json_cases.synthetic_result(40 + i)["results_z"] for i in range(5)]
    rows = json_cases.dense(arrays, stride=int(sizes.sum()) + 3)
    for strict in (False, True):
        rc, want, _, want_lens = rows_host(sizes, rows, strict, stride=rows.shape[1])
        assert rc == 0
        stride = (wt.jsonRowBound(sizes) + 15) // 16 * 16 + 32
        d_rows = torch.from_numpy(rows).cuda()
        text = torch.full((5, stride), FILL, dtype=torch.uint8, device="cuda")
        lens = torch.full((5,), -7, dtype=torch.int64, device="cuda")
        _lib.check(lib.wc_json_rows_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_rows.data_ptr(), rows.shape[1], 5,
                                        _lib.ptr(sizes), len(sizes), int(strict), text.data_ptr(), stride, lens.data_ptr()))
        got, got_lens = text.cpu().numpy(), lens.cpu().numpy()
        assert np.array_equal(got_lens, want_lens)
        for i in range(5):
            assert got[i, :got_lens[i]].tobytes() == want[i]
            assert np.all(got[i, got_lens[i]:] == FILL)         # the header: bytes behind text_len[i] are not written
        # the library call's plain files are made of these rows
    files = wt.export_json_batch([json_cases.synthetic_result(40 + i) for i in range(2)])
    for i, data in enumerate(files):
        assert data == jr.file_text(json_cases.synthetic_result(40 + i))


def test_refusals_leave_the_outputs_untouched(wt):
    import torch
    from wisecondor_amd import _lib
    lib = _lib.load()
    sizes = [5, 0, 3]
    rows = np.ones((2, 8))
    bound = wt.jsonRowBound(sizes)

    def refused(code, sizes=sizes, rows=rows, stride=None, text_stride=None, n_rows=None):
        s = np.ascontiguousarray(sizes, dtype=np.int64)
        text = np.full((2, bound + 64), FILL, dtype=np.uint8)
        lens = np.full(2, -7, dtype=np.int64)
        rc = lib.wc_json_rows(_lib.context(0), _lib.ptr(rows), 8 if stride is None else stride, 2 if n_rows is None else n_rows, _lib.ptr(s),
                              len(s), 0, _lib.ptr(text), bound + 64 if text_stride is None else text_stride, _lib.ptr(lens), None)
        assert rc == code, (rc, lib.wc_last_error())
        assert np.all(text == FILL) and np.all(lens == -7)

    refused(_lib.E_ARG, sizes=[5, -1, 3])
    refused(_lib.E_ARG, n_rows=-1)
    refused(_lib.E_ARG, stride=7)
    refused(_lib.E_ARG, text_stride=bound - 1)
    refused(_lib.E_LIMIT, n_rows=65536)
    refused(_lib.E_LIMIT, sizes=[1] * 65)
    refused(_lib.E_LIMIT, sizes=[1 << 30, 1 << 30], stride=1 << 40, text_stride=1 << 50)
    assert rows_host(sizes, rows, text_stride=bound)[0] == 0
    # the device form also wants rows that start on multiples of 16
    s = np.ascontiguousarray(sizes, dtype=np.int64)
    d_rows = torch.ones((2, 8), dtype=torch.float64, device="cuda")
    stride = (bound + 15) // 16 * 16
    text = torch.full((2 * stride + 64,), FILL, dtype=torch.uint8, device="cuda")
    lens = torch.full((2,), -7, dtype=torch.int64, device="cuda")
    for shift, step, code in ((8, stride, _lib.E_ARG), (0, stride + 8, _lib.E_ARG), (0, stride - 16, _lib.E_ARG)):
        rc = lib.wc_json_rows_dev(_lib.context(0), torch.cuda.current_stream().cuda_stream, d_rows.data_ptr(), 8, 2, _lib.ptr(s), 3, 0,
                                  text.data_ptr() + shift, step, lens.data_ptr())
        assert rc == code, (rc, lib.wc_last_error())
    torch.cuda.synchronize()
    assert bool((text == FILL).all()) and bool((lens == -7).all())
    assert lib.wc_format_doubles(_lib.context(0), None, -1, 0, None, None) == _lib.E_ARG


def _write_results(tmp_path, seeds, sizes_of=lambda seed: None):
    from wisecondor_amd import wisecondor as cli
    paths, results = [], []
    for seed in seeds:
        res = json_cases.synthetic_result(seed, sizes=sizes_of(seed), n_calls=seed % 3)
        path = str(tmp_path / ("s%d_test.npz" % seed))
        cli.write_npz(path, arguments=res["arguments"], runtime={"host": "x"}, binsize=res["binsize"],
                      results_r=cli._as_object_array(res["results_r"]), results_z=cli._as_object_array(res["results_z"]),
                      results_cwz=res["results_cwz"], results_calls=res["results_calls"], threshold_z=res["threshold_z"],
                      asdef=res["asdef"], aasdef=res["aasdef"])
        paths.append(path)
        results.append(res)
    return paths, results


def _read_back(data, path):
    back = json.loads(data)
    with np.load(path, allow_pickle=True, encoding="latin1") as f:
        for key in ("results_z", "results_r"):
            assert len(back[key]) == len(f[key])
            for got, want in zip(back[key], f[key]):
                assert jr.same_bits(got, want)
        assert jr.same_bits(back["results_cwz"], f["results_cwz"])
        calls = np.asarray(f["results_calls"], dtype=np.float64).reshape(-1, 5)
        assert jr.same_bits(np.array(back["results_calls"], dtype=np.float64).reshape(-1, 5), calls)
        assert back["binsize"] == f["binsize"].item() and back["threshold_z"] == f["threshold_z"].item()
        assert back["asdef"] == f["asdef"].item() and back["aasdef"] == f["aasdef"].item()
    assert "func" not in back["arguments"] and "nested" not in back["arguments"] and back["arguments"]["repeats"] == 5


def test_exportjson_command_line(tmp_path, capsys):
    """Five files in batches of two: one cannot be read, one has other chromosome lengths."""
    from wisecondor_amd import wisecondor as cli
    other = list(json_cases.SIZES)
    other[4] += 1
    paths, results = _write_results(tmp_path, [1, 2, 3, 4], sizes_of=lambda seed: other if seed == 3 else None)
    damaged = str(tmp_path / "damaged_test.npz")
    with open(damaged, "wb") as f:
        f.write(open(paths[0], "rb").read()[:200])
    outdir = tmp_path / "json"
    with pytest.raises(SystemExit) as stop:
        cli.main(["exportjson", paths[0], damaged, paths[1], paths[2], paths[3], str(outdir), "-batch", "2"])
    assert stop.value.code == 1
    said = capsys.readouterr().out
    assert "damaged_test.npz skipped: cannot be read" in said and "s3_test.npz skipped: other chromosome lengths" in said
    assert "3 files written" in said
    assert sorted(os.listdir(str(outdir))) == ["s1_test.json", "s2_test.json", "s4_test.json"]
    for seed, path, res in zip((1, 2, 3, 4), paths, results):
        if seed == 3:
            continue
        data = open(str(outdir / ("s%d_test.json" % seed)), "rb").read()
        assert data == jr.file_text(res)
        _read_back(data, path)


@pytest.mark.parametrize("strict", [False, True])
def test_exportjson_command_line_gz(tmp_path, capsys, strict):
    from wisecondor_amd import wisecondor as cli
    paths, results = _write_results(tmp_path, [5, 6, 7])
    plain, packed = tmp_path / "plain", tmp_path / "packed"
    extra = ["-strict"] if strict else []
    cli.main(["exportjson"] + paths + [str(plain), "-batch", "2"] + extra)
    cli.main(["exportjson"] + paths + [str(packed), "-batch", "2", "-gz"] + extra)
    capsys.readouterr()
    assert sorted(os.listdir(str(packed))) == ["s%d_test.json.gz" % s for s in (5, 6, 7)]
    for seed, path, res in zip((5, 6, 7), paths, results):
        data = open(str(plain / ("s%d_test.json" % seed)), "rb").read()
        assert data == jr.file_text(res, strict=strict)
        blob = open(str(packed / ("s%d_test.json.gz" % seed)), "rb").read()
        assert gzip.decompress(blob) == data            # (Python's gzip checks every member's CRC-32 and ISIZE)
        # three members, each read on its own
        import zlib
        members, rest = [], blob
        while rest:
            d = zlib.decompressobj(31)
            members.append(d.decompress(rest))
            assert d.eof
            rest = d.unused_data
        assert len(members) == 3 and members[1].startswith(b',"results_z":[[') and members[2].startswith(b',"results_r":[[')
        assert members[2].endswith(b"]]}") and members[0].startswith(b'{"binsize":')
        if strict:
            def refuse(name):
                raise AssertionError(name)
            json.loads(data, parse_constant=refuse)
        else:
            _read_back(data, path)


def test_gz_members_are_the_fixed_length_encoders_bytes(wt):
    """Each of the two GPU members of a -gz file is gzipAssemble(deflateRows(member input)), the member's input deflated
    on its own as one row of its own length (wc_deflate_rows_dev): the call that takes all rows with their lengths on
    the device writes the bytes the row-by-row calls wrote."""
    import torch
    results = [json_cases.synthetic_result(70 + i) for i in range(3)]
    files = wt.export_json_batch(results, gz=True)
    for res, blob in zip(results, files):
        whole = jr.file_text(res)
        z_at, r_at = whole.index(b',"results_z":'), whole.index(b',"results_r":')
        assert gzip.decompress(blob) == whole
        rest = blob
        for k, want in enumerate((whole[:z_at], whole[z_at:r_at], whole[r_at:])):
            d = zlib.decompressobj(31)
            assert d.decompress(rest) == want and d.eof
            member, rest = rest[:len(rest) - len(d.unused_data)], d.unused_data
            if k == 0:
                continue                    # (the host's part, through zlib)
            row = torch.from_numpy(np.frombuffer(want, dtype=np.uint8).copy()).cuda()[None, :]
            streams, lengths, crcs = wt.deflateRows(row)
            stream = streams[0, :int(lengths[0])].cpu().numpy()
            assert member == wt.gzipAssemble(stream, int(crcs[0].item()) & 0xffffffff, len(want)), k
        assert not rest


def test_a_batch_larger_than_one_call_comes_out_whole(wt):
    """export_json_batch splits at max_rows rows per GPU call (65 535, what wc_json_rows_dev accepts; here 4).  The
    deflate stage takes the rows of a GPU call in one call, their lengths read on the device, so it is split with them."""
    results = [json_cases.synthetic_result(60 + i) for i in range(5)]
    for gz in (False, True):
        files = wt.export_json_batch(results, gz=gz, max_rows=4)
        whole = wt.export_json_batch(results, gz=gz)
        assert files == whole and len(files) == 5
        for res, data in zip(results, files):
            assert (gzip.decompress(data) if gz else data) == jr.file_text(res)
