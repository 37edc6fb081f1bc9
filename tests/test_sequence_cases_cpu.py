"""What tests/sequence_cases.py promises, held without a GPU: the registry's shape, that the inputs are the same arrays
whenever they are made, that the LARGE shape of every job demands more of every workspace the job uses than the SMALL
one (so SMALL, LARGE, SMALL, LARGE on one context grows and then reuses), the sizes the scenarios of
tests/test_call_sequences_gpu.py rest on, and the comparison and the context swap themselves."""
import numpy as np
import pytest

import sequence_cases as sq


def test_registry():
    assert len(sq.JOBS) == 13 and len(set(sq.NAMES)) == 13
    for job in sq.JOBS:
        assert callable(job.run) and callable(job.demand) and sq.BY_NAME[job.name] is job


@pytest.mark.parametrize("name", sq.NAMES)
def test_large_demands_more_of_every_workspace(name):
    small, large = sq.BY_NAME[name].demand(sq.SMALL), sq.BY_NAME[name].demand(sq.LARGE)
    assert sorted(small) == sorted(large) and small
    for key in small:
        assert large[key] > small[key] > 0, (name, key, small[key], large[key])


def _flat(value):
    if isinstance(value, dict):
        return [x for k in sorted(value, key=str) for x in _flat(value[k])]
    if isinstance(value, (list, tuple)):
        return [x for v in value for x in _flat(v)]
    if isinstance(value, np.ndarray):
        return [(str(value.dtype), value.shape, value.tobytes())]
    return [value if not callable(value) else value.__name__]


INPUTS = [("newref_case", True), ("tp_layout", False), ("tp_samples", False), ("small_case", True), ("eigh_case", True),
          ("convert_case", True), ("deflate_case", True), ("export_case", True), ("plot_case", True), ("pdf_case", True),
          ("crossval_case", True)]


@pytest.mark.parametrize("maker, shaped", INPUTS, ids=[m for m, _ in INPUTS])
def test_inputs_are_deterministic(maker, shaped):
    fn = getattr(sq, maker)
    for args in ([(sq.SMALL,), (sq.LARGE,)] if shaped else [()]):
        first = _flat(fn(*args))
        fn.cache_clear()
        assert _flat(fn(*args)) == first and len(first) > 0
    if shaped:
        assert _flat(fn(sq.SMALL)) != _flat(fn(sq.LARGE))


def test_walks_are_deterministic_and_cover_the_registry():
    assert sq.walk_steps(3) == sq.walk_steps(3) != sq.walk_steps(4)
    steps = [s for seed in range(6) for s in sq.walk_steps(seed)]
    assert len(steps) == 240 and {n for n, _ in steps} == set(sq.NAMES) and {s for _, s in steps} == set(sq.SHAPES)


def test_shapes_the_scenarios_rest_on():
    """The pinned block: prep with one component leaves 8 B bytes, the same counts with eight components ask for 64 B,
    and the LARGE pdf job asks for more than prep's one component left -- each grows the block and nothing else.  The
    LARGE general batch pads its samples to 48; the latency job stays within the eight samples latency mode takes."""
    import prep_cases as pc
    s, b = sq.PREP_CASES[sq.SMALL]
    assert (s, b, 1) in pc.COMP_CASES and (s, b, 8) in pc.COMP_CASES and sq.PREP_COMPS == (1, 8)
    assert 8 * b > 256                                             # beyond the 256 bytes the test path asks for
    pages, panels = sq.PDF_PAGES[sq.LARGE], len(sq.pdf_case(sq.LARGE)[0]["chromosomes"])
    assert pages >= 65 and 4 * pages * panels > 8 * b > 4 * sq.PDF_PAGES[sq.SMALL] * len(sq.pdf_case(sq.SMALL)[0]["chromosomes"])
    assert sq.TEST_SAMPLES == {sq.SMALL: 12, sq.LARGE: 40} and -(-40 // 16) * 16 == 48
    assert max(sq.LAT_SAMPLES.values()) <= 8 and max(sq.TEST_SIZES) <= 2048
    assert len(sq.tp_samples()) >= 20 + max(sq.LAT_SAMPLES.values()) and len(sq.tp_samples()) >= max(sq.TEST_SAMPLES.values())
    lay = sq.tp_layout()
    assert lay["indexes"].shape == (sum(sq.TEST_SIZES), 40) and lay["indexes"].dtype == np.int32
    for res in sq.pdf_case(sq.LARGE)[1]:                           # one GPU call: one threshold, one set of lengths
        assert res["threshold_z"] == sq.pdf_case(sq.LARGE)[1][0]["threshold_z"]
        assert [len(c) for c in res["results_z"]] == [len(c) for c in sq.pdf_case(sq.LARGE)[1][0]["results_z"]]
    for shape in sq.SHAPES:
        assert len({tuple(len(c) for c in r["results_z"]) for r in sq.plot_case(shape)[1]}) == 1
        assert sq.DEFLATE[shape][1] > 0 and len(sq.sens_plan(shape)) == len(sq.SENS_ROWS[shape])
    assert sq.DEFLATE[sq.LARGE][1] > 65536 > sq.DEFLATE[sq.SMALL][1]


def test_same_compares_bits():
    nan_a = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)
    nan_b = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)
    assert sq.same({"x": nan_a, "b": b"ab"}, {"x": nan_a.copy(), "b": b"ab"}) is None
    assert "x" in sq.same({"x": nan_a}, {"x": nan_b})                     # NaN payloads count
    assert "x" in sq.same({"x": np.array([0.0])}, {"x": np.array([-0.0])})
    assert "x" in sq.same({"x": np.zeros(2, np.int32)}, {"x": np.zeros(2, np.int64)})
    assert "x" in sq.same({"x": np.zeros((2, 1))}, {"x": np.zeros((1, 2))})
    assert "b" in sq.same({"b": b"ab"}, {"b": b"ac"}) and "b" in sq.same({"b": b"ab"}, {"b": b"abc"})
    assert "keys" in sq.same({"x": b""}, {"y": b""})


def test_the_context_swap_puts_back_what_was():
    from wisecondor_amd import _lib
    saved = dict(_lib._contexts)
    try:
        _lib._contexts.clear()
        with sq.on_context(1234):
            assert _lib._contexts == {0: 1234}
        assert _lib._contexts == {}
        _lib._contexts[0] = 99
        with pytest.raises(KeyError):
            with sq.on_context(1234):
                with sq.on_context(5678):
                    assert _lib._contexts[0] == 5678
                assert _lib._contexts[0] == 1234
                raise KeyError("from inside")
        assert _lib._contexts == {0: 99}
    finally:
        _lib._contexts.clear()
        _lib._contexts.update(saved)


def test_the_environment_switch_puts_back_what_was(monkeypatch):
    import os
    monkeypatch.setenv("WC_TEST_LATENCY_MODE", "2")
    with sq.environ(WC_TEST_LATENCY_MODE=None):
        assert "WC_TEST_LATENCY_MODE" not in os.environ
    assert os.environ["WC_TEST_LATENCY_MODE"] == "2"
    with sq.environ(WC_TEST_LATENCY_MODE="0"):
        assert os.environ["WC_TEST_LATENCY_MODE"] == "0"
    assert os.environ["WC_TEST_LATENCY_MODE"] == "2"
