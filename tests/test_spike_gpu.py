"""k_spike and k_spike_score (csrc/spike.hip) by bits against the restatement (spike_restated.py).

The spike: rows of 1021 .. 1024 bins (n_total % 4 takes every value, so a trial's row begins at every place against a
16-byte store), 1, 2 and 257 trials from 1 and 3 base rows named out of order and more than once, spans at every
alignment of both ends, every edge of the flat array, the rounding ties, the saturation edge and negative counts; the
device form also with the output and the base rows beginning at every multiple of four bytes.  Output buffers are
pre-filled with 0x5A and end in a guard row that must stay as it is.  The score: hand-written call lists in rooms of
1, 64, 65 and 300 rows."""
import numpy as np
import pytest

import spike_restated as sr

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A
PPM = [-1000000, -999999, -1, 0, 1, 499999, 500000, 2500000, 100000000]
COUNTS = [0, 1, 2, 3, 21262214, 21474837, 2 ** 31 - 1, -5]


@pytest.fixture(scope="module")
def env():
    import torch
    from wisecondor_amd import _lib, sensitivity
    return dict(torch=torch, lib=_lib.load(), _lib=_lib, se=sensitivity, ctx=_lib.context(0))


def sizes_of(r):
    return np.array([5, 3, 1, 1012 + r], dtype=np.int64)


def base_rows(n_base, n_total, seed):
    """Poisson(30) counts; every special count at bins 20 .. 27 of the long chromosome (flat 29 .. 36) and, at random,
    behind flat bin 60 (the spans that try every alignment lie in plain counts: every one of their bins changes)."""
    rng = np.random.RandomState(seed)
    base = rng.poisson(30, size=(n_base, n_total)).astype(np.int64) + 1
    special = rng.rand(n_base, n_total) < 0.3
    special[:, :60] = False
    base[special] = rng.choice(COUNTS, size=int(special.sum()))
    base[:, 29:29 + len(COUNTS)] = COUNTS
    return base.astype(np.int32)


STRONG = [2500000, -1000000, 100000000, 500000]       # every count >= 1 changes


def plan_of(n_trials, n_base, r, seed):
    """Trial 0 spikes the array's first element and the last trial its last one.  Between them: spans on the long
    chromosome at every start 0 .. 7 x every length 1 .. 9, the special counts under every ppm value, the whole one-bin
    chromosome, whole chromosomes, and spans drawn at random under the ppm values in rotation."""
    rng = np.random.RandomState(seed)
    long_size = 1012 + r
    if n_trials == 1:
        return np.array([[0, 1, 0, 5, 2500000]], dtype=np.int32)
    spans = [(4, first, bins, STRONG[(first + bins) % 4]) for first in range(8) for bins in range(1, 10)]
    spans += [(4, 20, 8, ppm) for ppm in PPM]
    spans += [(3, 0, 1, 2500000), (1, 0, 5, -1000000), (2, 0, 3, 500000), (4, 0, long_size, 2500000), (4, long_size - 9, 9, 100000000),
              (2, 2, 1, 0)]
    while len(spans) < n_trials - 2:
        bins = int(rng.randint(1, 200))
        spans.append((4, int(rng.randint(0, long_size - bins + 1)), bins, PPM[len(spans) % len(PPM)]))
    middle = spans[:n_trials - 2]
    rows = [(1, 0, 1, 100000000)] + middle + [(4, long_size - 1, 1, 2500000)]
    # base rows out of order and more than once
    return np.array([((n_base - 1 - i) % n_base if i % 3 else (i // 3) % n_base,) + row for i, row in enumerate(rows)], dtype=np.int32)


SHAPES = [(n_trials, n_base, r) for r in range(4) for n_trials, n_base in ((1, 1), (2, 3), (257, 3), (257, 1))]


@pytest.mark.parametrize("n_trials, n_base, r", SHAPES)
def test_spike_counts_host_form(env, n_trials, n_base, r):
    sizes = sizes_of(r)
    base = base_rows(n_base, int(sizes.sum()), 10 + r)
    plan = plan_of(n_trials, n_base, r, 20 + r)
    want, want_saturated = sr.spike(base, sizes, plan)
    got, saturated = env["se"].spikeCounts(base, sizes, plan)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert saturated == want_saturated
    if n_trials == 257:
        assert want_saturated > 0 and (want != base[plan[:, 0]]).any()
        assert len(set(plan[:, 0].tolist())) == n_base and set(plan[:, 4].tolist()) == set(PPM)
        again, _ = env["se"].spikeCounts(base, sizes, plan)
        assert np.array_equal(again, want)
        fewer, _ = env["se"].spikeCounts(base, sizes, plan[:5])
        assert np.array_equal(fewer, want[:5])
        assert np.array_equal(env["se"].spikeCounts(base, sizes, plan)[0], want)


def run_dev(env, base, sizes, plan, out_shift=0, base_shift=0):
    """wc_spike_counts_dev with the output `out_shift` and the base rows `base_shift` elements behind a 16-byte address;
    (rc, the output rows, the guard row and the elements in front, saturated)."""
    torch, lib = env["torch"], env["lib"]
    n_total, n = int(sizes.sum()), len(plan)
    room = torch.full((out_shift + (n + 1) * n_total,), FILL, dtype=torch.int32, device="cuda")
    src = torch.zeros((base_shift + base.size,), dtype=torch.int32, device="cuda")
    src[base_shift:] = torch.from_numpy(base.ravel()).cuda()
    sat = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    assert room.data_ptr() % 16 == 0 and src.data_ptr() % 16 == 0
    rc = lib.wc_spike_counts_dev(env["ctx"], None, src.data_ptr() + 4 * base_shift, base.shape[0], env["_lib"].ptr(sizes), len(sizes),
                                 env["_lib"].ptr(plan), n, room.data_ptr() + 4 * out_shift, sat.data_ptr())
    torch.cuda.synchronize()
    host = room.cpu().numpy()
    return rc, host[out_shift:out_shift + n * n_total].reshape(n, n_total), np.concatenate([host[:out_shift], host[out_shift + n * n_total:]]), \
        int(sat.item())


@pytest.mark.parametrize("n_trials, n_base, r", SHAPES)
def test_spike_counts_device_form_at_every_alignment(env, n_trials, n_base, r):
    sizes = sizes_of(r)
    base = base_rows(n_base, int(sizes.sum()), 30 + r)
    plan = plan_of(n_trials, n_base, r, 40 + r)
    want, want_saturated = sr.spike(base, sizes, plan)
    for out_shift, base_shift in ((0, 0), (1, 0), (2, 3), (3, 1), (0, 2)):
        rc, got, guard, saturated = run_dev(env, base, sizes, plan, out_shift, base_shift)
        assert rc == 0, env["lib"].wc_last_error()
        assert np.array_equal(got, want), (out_shift, base_shift, np.argwhere(got != want)[:5])
        assert (guard == FILL).all(), (out_shift, base_shift)
        assert saturated == want_saturated


def test_spike_rows_shorter_than_a_store(env):
    """One, two and three bins in a row: several trials share a 16-byte store."""
    for sizes in ([1], [2], [1, 2], [3]):
        sizes = np.array(sizes, dtype=np.int64)
        n_total = int(sizes.sum())
        base = np.array([[7, 2 ** 31 - 1, 1][:n_total], [3, 0, -5][:n_total]], dtype=np.int32)
        plan = np.array([[i % 2, len(sizes), 0, int(sizes[-1]), PPM[i % len(PPM)]] for i in range(11)], dtype=np.int32)
        want, want_saturated = sr.spike(base, sizes, plan)
        for out_shift in range(4):
            rc, got, guard, saturated = run_dev(env, base, sizes, plan, out_shift, 0)
            assert rc == 0 and np.array_equal(got, want) and (guard == FILL).all() and saturated == want_saturated


def test_spike_rows_longer_than_one_workgroups_share(env):
    """A workgroup takes 1 024 quads of a row: rows of 4 107 .. 4 110 bins need a second one, and spans lie across the
    seam (flat bins 4 096 +- 4 of the row, at every output alignment) and on the row's last bins."""
    for r in range(4):
        sizes = np.array([7, 4100 + r], dtype=np.int64)
        n_total = int(sizes.sum())
        base = base_rows(2, n_total, 60 + r)
        plan = np.array([[1, 2, 4080, 20, 2500000], [0, 2, 4089 - 7, 1, 100000000], [1, 2, 4085, 8 + r, -1000000],
                         [0, 2, 0, 4100 + r, 500000], [1, 2, 4099 + r, 1, 2500000], [0, 1, 0, 7, 2500000]], dtype=np.int32)
        want, want_saturated = sr.spike(base, sizes, plan)
        assert (want[:, 4090:4100] != base[plan[:, 0]][:, 4090:4100]).any()
        for out_shift in range(4):
            rc, got, guard, saturated = run_dev(env, base, sizes, plan, out_shift, (out_shift + r) % 4)
            assert rc == 0 and np.array_equal(got, want) and (guard == FILL).all() and saturated == want_saturated


@pytest.mark.parametrize("bad, row", [
    ((3, 4, 0, 1, 5), "base row 3"), ((-1, 4, 0, 1, 5), "base row -1"), ((0, 0, 0, 1, 5), "chromosome 0"), ((0, 5, 0, 1, 5), "chromosome 5"),
    ((0, 4, -1, 1, 5), "first bin -1"), ((0, 4, 0, 0, 5), "0 bins"), ((0, 4, 1000, 13, 5), "bins 1000 .. 1012"),
    ((0, 3, 0, 2, 5), "bins 0 .. 1"), ((0, 4, 0, 1, -1000001), "-1000001 ppm"), ((0, 4, 0, 1, 100000001), "100000001 ppm"),
    ((0, 4, 2147483647, 2147483647, 5), "plan row 6"),
])
def test_spike_refusals_name_the_row_and_leave_the_output(env, bad, row):
    sizes = sizes_of(0)
    base = base_rows(3, int(sizes.sum()), 50)
    plan = plan_of(9, 3, 0, 51)
    plan[6] = bad
    rc, got, guard, saturated = run_dev(env, base, sizes, plan)
    message = env["lib"].wc_last_error().decode()
    assert rc == env["_lib"].E_ARG
    assert "plan row 6" in message and row in message, message
    assert (got == FILL).all() and (guard == FILL).all() and saturated == -7
    out = np.full((9, int(sizes.sum())), FILL, dtype=np.int32)
    rc = env["lib"].wc_spike_counts(env["ctx"], env["_lib"].ptr(base), 3, env["_lib"].ptr(sizes), 4, env["_lib"].ptr(plan), 9,
                                    env["_lib"].ptr(out), None)
    assert rc == env["_lib"].E_ARG and (out == FILL).all()
    rc = env["lib"].wc_spike_counts(env["ctx"], env["_lib"].ptr(base), 3, env["_lib"].ptr(sizes), 4, env["_lib"].ptr(plan), 0,
                                    env["_lib"].ptr(out), None)
    assert rc == env["_lib"].E_ARG and (out == FILL).all()


# ------------------------------------------------------------------------------------------- the score ----
GAIN, LOSS, CONTROL = (0, 2, 10, 5, 50000), (1, 2, 10, 5, -50000), (0, 2, 10, 5, 0)      # span 10 .. 14 of chromosome 2
NAN = float("nan")
FAR = [7.0, 100.0, 120.0, 9.0, 0.5]                       # a call elsewhere


def score_cases(room):
    """(plan row, call rows) of every case that fits `room` rows."""
    cases = [
        (GAIN, [[2, 6, 10, 7.0, 0.1]]),                                          # touches the span's first bin
        (GAIN, [[2, 14, 20, 7.0, 0.1]]),                                         # ... its last bin
        (LOSS, [[2, 14, 14, -7.0, -0.1]]),
        (GAIN, [[2, 5, 9, 7.0, 0.1]]),                                           # adjacent on either side: no match
        (GAIN, [[2, 15, 20, 7.0, 0.1]]),
        (GAIN, [[2, 10, 14, -7.0, -0.1]]),                                       # the span, the wrong sign
        (LOSS, [[2, 10, 14, 7.0, 0.1]]),
        (GAIN, [[3, 10, 14, 7.0, 0.1]]),                                         # the span, the wrong chromosome
        (GAIN, [[2, 10, 14, NAN, 0.1]]), (LOSS, [[2, 10, 14, NAN, 0.1]]),
        (GAIN, [[2, 10, 14, 0.0, 0.1]]), (LOSS, [[2, 10, 14, -0.0, 0.1]]), (GAIN, [[2, 10, 14, -0.0, 0.1]]),
        (CONTROL, [[2, 10, 14, 7.0, 0.1]]), (CONTROL, [[2, 10, 14, -7.0, 0.1]]),
        (GAIN, []), (LOSS, []),
        (GAIN, [[2, 10, 14, 7.5, 0.25]]),
        (GAIN, [[2, 0, 1000, 7.5, NAN]]),                                        # a call around the span; its effect is copied as it is
    ]
    if room >= 2:
        cases += [(GAIN, [[2, 9, 11, 6.0, 0.1], [2, 13, 15, 8.0, 0.2]]),                     # tied overlaps: the earlier row
                  (GAIN, [FAR, [2, 13, 15, 8.0, 0.2]]), (LOSS, [[2, 12, 13, 8.0, 0.2], [2, 12, 13, -8.0, -0.2]])]
    if room >= 4:
        cases += [(GAIN, [[2, 8, 10, 6.0, 0.1], FAR, [2, 11, 12, 6.5, 0.2], [2, 12, 20, 8.0, 0.3]]),       # the largest overlap last
                  (CONTROL, [FAR, [2, 11, 12, 6.5, 0.2], [2, 12, 20, -8.0, 0.3], FAR])]
    if room >= 64:
        cases += [(GAIN, [FAR] * 63 + [[2, 10, 12, 6.0, 0.4]]),                              # the only match in the last lane
                  (GAIN, [[2, 14, 30, 6.0, 0.4]] + [FAR] * 62 + [[2, 0, 10, 6.5, 0.4]])]    # a tie of lane 0 and lane 63
    if room >= 65:
        cases += [(GAIN, [FAR] * 64 + [[2, 10, 12, 6.0, 0.4]]),                              # ... in the second pass
                  (GAIN, [[2, 14, 30, 6.0, 0.4]] + [FAR] * 63 + [[2, 0, 10, 6.5, 0.4]]),    # a tie within lane 0: the earlier row
                  (GAIN, [[2, 14, 30, 6.0, 0.4]] + [FAR] * 63 + [[2, 0, 11, 6.5, 0.4]])]    # the later row with the larger overlap
    if room >= 300:
        cases += [(GAIN, [FAR] * 299 + [[2, 12, 13, 6.0, 0.4]]),                             # the only match in row 299
                  (LOSS, [[2, 10 + i % 5, 10 + i % 5, -6.0 - i, -0.1] if i % 7 == 3 else FAR for i in range(300)])]
    full = [FAR] * (room - 1) + [[2, 13, 40, 6.0, 0.4]]                                      # n_calls = max_calls
    return cases + [(GAIN, full)]


def score_inputs(room):
    cases = score_cases(room)
    plan = np.array([c[0] for c in cases], dtype=np.int32)
    calls = np.empty((len(cases), room, 5), dtype=np.float64)
    # rows at and behind n_calls: calls that would match the span if they were read
    calls[:] = [2.0, 10.0, 14.0, 9.0, 1.0]
    calls[plan[:, 4] < 0, :, 3] = -9.0
    n_calls = np.array([len(c[1]) for c in cases], dtype=np.int32)
    for i, (_, rows) in enumerate(cases):
        if rows:
            calls[i, :len(rows)] = np.array(rows, dtype=np.float64)
    return plan, calls, n_calls


def same_records(got_i, got_f, want_i, want_f):
    assert np.array_equal(got_i, want_i), np.argwhere(got_i != want_i)[:5]
    nan = np.isnan(want_f)
    assert np.array_equal(np.isnan(got_f), nan)
    assert np.array_equal(got_f.view(np.int64)[~nan], want_f.view(np.int64)[~nan])


@pytest.mark.parametrize("room", [1, 64, 65, 300])
def test_score_host_and_device_forms(env, room):
    torch, lib = env["torch"], env["lib"]
    plan, calls, n_calls = score_inputs(room)
    want_i, want_f = sr.score(plan, calls, n_calls)
    assert (want_i[:, 1] > 0).any() and (want_i[:, 1] == 0).any() and n_calls.max() == room and n_calls.min() == 0
    got_i, got_f = env["se"].scoreTrials(plan, calls, n_calls)
    same_records(got_i, got_f, want_i, want_f)
    n = len(plan)
    rec_i = torch.full(((n + 1) * 8,), FILL, dtype=torch.int32, device="cuda")
    rec_f = torch.full(((n + 1) * 4,), FILL, dtype=torch.int32, device="cuda")         # (n + 1) * 2 doubles
    d_calls, d_n = torch.from_numpy(calls).cuda(), torch.from_numpy(n_calls).cuda()
    rc = lib.wc_spike_score_dev(env["ctx"], None, env["_lib"].ptr(plan), n, d_calls.data_ptr(), d_n.data_ptr(), room,
                                rec_i.data_ptr(), rec_f.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.wc_last_error()
    host_i, host_f = rec_i.cpu().numpy(), rec_f.cpu().numpy()
    same_records(host_i[:n * 8].reshape(n, 8), host_f[:n * 4].view(np.float64).reshape(n, 2), want_i, want_f)
    assert (host_i[n * 8:] == FILL).all() and (host_f[n * 4:] == FILL).all()


def test_score_designed_records(env):
    """A few records spelled out, so that the restatement is not the only witness."""
    plan, calls, n_calls = score_inputs(4)
    got_i, got_f = env["se"].scoreTrials(plan, calls, n_calls)
    cases = score_cases(4)
    tied = [i for i, c in enumerate(cases) if c[1] and c[1][0][:3] == [2, 9, 11]][0]
    assert got_i[tied].tolist() == [2, 2, 4, 6, 0, 9, 11, 0] and got_f[tied].tolist() == [6.0, 0.1]
    last = [i for i, c in enumerate(cases) if len(c[1]) == 4 and c[0] == GAIN and c[1][0][:3] == [2, 8, 10]][0]
    assert got_i[last].tolist() == [4, 3, 1 + 2 + 3, 3 + 2 + 9, 3, 12, 20, 0] and got_f[last].tolist() == [8.0, 0.3]
    assert got_i[0].tolist() == [1, 1, 1, 5, 0, 6, 10, 0]
    control = [i for i, c in enumerate(cases) if c[0] == CONTROL and len(c[1]) == 4][0]
    assert got_i[control].tolist() == [4, 0, 0, 0, -1, -1, -1, 0] and np.isnan(got_f[control]).all()


def test_score_refusals(env):
    plan, calls, n_calls = score_inputs(4)
    for bad, word in (((0, 2, -1, 5, 5), "first bin -1"), ((0, 2, 0, 0, 5), "0 bins"), ((0, 0, 0, 1, 5), "chromosome 0"),
                      ((0, 2, 0, 1, 100000001), "100000001 ppm")):
        broken = plan.copy()
        broken[2] = bad
        rec_i = np.full((len(plan), 8), FILL, dtype=np.int32)
        rec_f = np.zeros((len(plan), 2))
        rc = env["lib"].wc_spike_score(env["ctx"], env["_lib"].ptr(broken), len(plan), env["_lib"].ptr(calls), env["_lib"].ptr(n_calls), 4,
                                       env["_lib"].ptr(rec_i), env["_lib"].ptr(rec_f))
        message = env["lib"].wc_last_error().decode()
        assert rc == env["_lib"].E_ARG and "plan row 2" in message and word in message, message
        assert (rec_i == FILL).all()
