"""exportjson without a GPU: the digit routine on the host against CPython byte for byte, the file's restatement read
back by bits, the `arguments` filter, the command line's options, and the gzip members."""
import gzip
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import json_cases  # noqa: E402
import json_restated as jr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from wisecondor_amd import build, _lib
    build.build_library(verbose=False)
    return _lib.load()


def format_host(lib, values, strict):
    from wisecondor_amd import _lib
    v = np.ascontiguousarray(values, dtype=np.float64)
    text = np.full((len(v), 24), 0x55, dtype=np.uint8)
    lens = np.zeros(len(v), dtype=np.uint8)
    assert lib.wc_format_doubles_host(_lib.ptr(v), len(v), int(strict), _lib.ptr(text), _lib.ptr(lens)) == 0
    return text, lens


def first_differences(got, want, values, limit=5):
    at = np.nonzero(got != want)[0][:limit]
    return [(values[i].hex(), want[i], got[i]) for i in at]


@pytest.mark.parametrize("strict", [False, True])
def test_host_digits_equal_cpython_byte_for_byte(lib, strict):
    values = json_cases.digit_inputs()
    want = json_cases.digit_expected(strict)
    assert len(values) >= 1200000
    text, lens = format_host(lib, values, strict)
    got = text.reshape(-1).view("S24")
    assert not first_differences(got, want, values)
    assert np.array_equal(lens, np.char.str_len(want))
    # (an 'S24' comparison ignores trailing zero bytes: the padding is checked on its own)
    assert np.array_equal(text != 0, np.arange(24)[None, :] < lens[:, None])
    if strict:
        bad = ~np.isfinite(values)
        assert bad.sum() >= 7 and np.all(want[bad] == b"null")
    else:
        assert {b"NaN", b"Infinity", b"-Infinity", b"-0.0", b"0.0", b"5e-324", b"1e+16", b"1000000000000000.0", b"1e-05", b"0.0001",
                b"1e+22", b"1e+23", b"0.30000000000000004", b"1.7976931348623157e+308", b"123456789012345.6"} <= set(want.tolist())
        assert lens.max() == 24


def test_the_committed_table_is_what_the_generator_writes():
    assert subprocess.call([sys.executable, os.path.join(ROOT, "tools", "make_fmt_tables.py"), "--check"]) == 0


def test_restated_file_reads_back_by_bits(lib):
    from wisecondor_amd import wisetools as wt
    res = json_cases.synthetic_result(1)
    assert len(res["results_z"]) == 22 and 0 in json_cases.SIZES and 1 in json_cases.SIZES and len(res["results_calls"]) == 3
    flat = np.concatenate(res["results_z"])
    assert np.isnan(flat).any() and np.isinf(flat).any() and np.signbit(flat[flat == 0]).any()
    text = jr.file_text(res)
    back = json.loads(text)
    assert list(back) == list(jr.KEYS)
    for key in ("results_z", "results_r"):
        assert [len(c) for c in back[key]] == json_cases.SIZES
        for got, want in zip(back[key], res[key]):
            assert jr.same_bits(got, want)
    assert np.isnan(back["results_z"][0][3]) and back["results_z"][0][2] == float("inf")
    assert jr.same_bits(back["results_cwz"], res["results_cwz"])
    assert jr.same_bits([c[3:] for c in back["results_calls"]], res["results_calls"][:, 3:])
    assert [c[:3] for c in back["results_calls"]] == res["results_calls"][:, :3].astype(int).tolist()
    assert back["binsize"] == 250000 and isinstance(back["binsize"], int) and back["threshold_z"] == res["threshold_z"]
    # strict: nothing in the text that is not JSON
    def refuse(name):
        raise AssertionError("strict text holds %s" % name)
    strict = json.loads(jr.file_text(res, strict=True), parse_constant=refuse)
    assert strict["results_z"][0][2] is None and strict["results_z"][0][3] is None and strict["results_cwz"][1] is None
    with pytest.raises(AssertionError):
        json.loads(text, parse_constant=refuse)
    # the product's host part is the restatement's, and a row made of the host routine's digits is the restated row
    for mode in (False, True):
        whole = jr.file_text(res, strict=mode)
        head = wt.jsonHead(res, strict=mode)
        assert whole.startswith(head + b',"results_z":[[')
        row = np.concatenate(res["results_z"])
        digits = wt.formatDoubles(row, strict=mode)
        parts, at = [], 0
        for n in json_cases.SIZES:
            parts.append(b"[" + b",".join(digits[at:at + n]) + b"]")
            at += n
        assert b"[" + b",".join(parts) + b"]" == jr.row_text(row, json_cases.SIZES, strict=mode)
    empty = dict(res, results_calls=np.array([]))
    assert b'"results_calls":[]' in wt.jsonHead(empty) and json.loads(jr.file_text(empty))["results_calls"] == []


def test_row_bound(lib):
    from wisecondor_amd import wisetools as wt
    assert wt.jsonRowBound([]) == 2 and wt.jsonRowBound([0]) == 4 and wt.jsonRowBound([3, 0, 1]) == 25 * 4 + 2 * 3 + 2
    # "[]," is three bytes: every empty chromosome beyond the first takes one more than two
    assert wt.jsonRowBound([0, 0, 0]) == len("[[],[],[]]") and wt.jsonRowBound([0, 2, 0, 0]) == 50 + 8 + 2 + 2
    for sizes in ([5], [1, 1], [0, 3], [2, 0, 2], [0, 0, 1, 0]):
        longest = jr.row_text(np.full(sum(sizes), -1.2345678901234567e-308), sizes)
        assert len(longest) <= wt.jsonRowBound(sizes) <= len(longest) + 1
    with pytest.raises(ValueError):
        wt.jsonRowBound([3, -1])
    with pytest.raises(ValueError):
        wt.jsonRowBound([1] * 65)


def test_arguments_filter():
    from wisecondor_amd import wisetools as wt
    given = {"func": test_arguments_filter, "n": np.int64(3), "x": np.float64(0.5), "flag": np.bool_(True), "list": [1, "a", None, 2.5],
             "tuple": (1, 2), "nested": {"a": 1}, "mixed": [1, {"b": 2}], "array": np.arange(3), "none": None, "text": "s", "b": False}
    kept = wt.jsonArguments(given)
    assert kept == {"b": False, "flag": True, "list": [1, "a", None, 2.5], "n": 3, "none": None, "text": "s", "tuple": [1, 2], "x": 0.5}
    assert list(kept) == sorted(kept)
    assert type(kept["n"]) is int and type(kept["x"]) is float and type(kept["flag"]) is bool
    for key, value in given.items():
        assert (key in kept) == jr.plain(value)[0]
    json.dumps(kept, allow_nan=False)


def test_options_and_duplicate_stems(tmp_path, capsys):
    from wisecondor_amd import ingest
    from wisecondor_amd import wisecondor as cli
    p = cli.buildParser()
    a = p.parse_args(["exportjson", "a_test.npz", "b_test.npz", "out"])
    assert (a.infiles, a.outdir, a.strict, a.gz, a.batch, a.io) == (["a_test.npz", "b_test.npz"], "out", False, False, 64, 8)
    assert a.func is cli.toolExportJson
    a = p.parse_args(["exportjson", "a.npz", "out", "-strict", "-gz", "-batch", "2", "-io", "3"])
    assert (a.strict, a.gz, a.batch, a.io) == (True, True, 2, 3)
    assert ingest.export_output_names(["x/a_test.npz", "b"], "o") == [os.path.join("o", "a_test.json"), os.path.join("o", "b.json")]
    assert ingest.export_output_names(["a.npz"], "o", gz=True) == [os.path.join("o", "a.json.gz")]
    outdir = tmp_path / "never"
    with pytest.raises(SystemExit) as stop:
        cli.main(["exportjson", str(tmp_path / "one" / "s_test.npz"), str(tmp_path / "two" / "s_test.npz"), str(outdir)])
    assert stop.value.code == 2 and not outdir.exists()
    assert "would both be written to s_test.json" in capsys.readouterr().out


def test_gzip_members(lib):
    from wisecondor_amd import _lib
    from wisecondor_amd import wisetools as wt
    rng = np.random.RandomState(5)
    inputs = [b"", b"x", bytes(rng.randint(48, 58, size=70000).astype(np.uint8)), b'{"a":[1.0,2.5]}' * 40]
    members = []
    for raw in inputs:
        packer = zlib.compressobj(6, zlib.DEFLATED, -15)
        stream = packer.compress(raw) + packer.flush()
        member = wt.gzipAssemble(stream, zlib.crc32(raw), len(raw))
        assert len(member) == len(stream) + 18 == lib.wc_gzip_bytes(len(stream))
        assert member[:10] == bytes([0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 255]) and member[10:-8] == stream
        assert gzip.decompress(member) == raw
        assert wt.gzipAssemble(stream, zlib.crc32(raw), len(raw)) == member
        members.append(member)
    assert gzip.decompress(members[3] + members[2] + members[1]) == inputs[3] + inputs[2] + inputs[1]
    assert gzip.decompress(b"".join(members)) == b"".join(inputs)
    # a wrong checksum or length is Python's to find
    packer = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = packer.compress(inputs[3]) + packer.flush()
    with pytest.raises(Exception):
        gzip.decompress(wt.gzipAssemble(stream, zlib.crc32(inputs[3]) ^ 1, len(inputs[3])))
    with pytest.raises(Exception):
        gzip.decompress(wt.gzipAssemble(stream, zlib.crc32(inputs[3]), len(inputs[3]) + 1))
    # too little room is refused and nothing is written
    src = np.frombuffer(stream, dtype=np.uint8).copy()
    out = np.full(len(src) + 18, 0x55, dtype=np.uint8)
    n = np.full(1, -7, dtype=np.int64)
    for cap in (len(src) + 17, 0, -1):
        assert lib.wc_gzip_assemble(_lib.ptr(src), len(src), 0, 5, _lib.ptr(out), cap, _lib.ptr(n)) == _lib.E_ARG
        assert np.all(out == 0x55) and n[0] == -7
    assert lib.wc_gzip_assemble(_lib.ptr(src), len(src), 0, -1, _lib.ptr(out), len(out), _lib.ptr(n)) == _lib.E_ARG
    assert lib.wc_gzip_bytes(-1) == -1
