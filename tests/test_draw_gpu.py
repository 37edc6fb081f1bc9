"""The draw kernels (csrc/draw.hip) by bits against the restatement (draw_restated.py, inputs in draw_cases.py): the
known-answer kernel, k_thin in both of its forms (a lane per bin, a wave per bin from the cutoff on) and the binomial
spike (k_spike's copy and k_draw_patch).  Output buffers are pre-filled with 0x5A and end in a guard row that must stay
as it is."""
import numpy as np
import pytest

import draw_cases as dc
import draw_restated as dr
import spike_restated as sr

pytestmark = pytest.mark.gpu
FILL = 0x5A5A5A5A
KNOWN = [([0, 0, 0, 0], [0, 0], "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], "d16cfe09 94fdcceb 5001e420 24126ea1")]


@pytest.fixture(scope="module")
def env():
    import torch
    from wisecondor_amd import _lib, sensitivity
    return dict(torch=torch, lib=_lib.load(), _lib=_lib, se=sensitivity, ctx=_lib.context(0))


def device_words(env, counters, keys):
    counters = np.ascontiguousarray(counters, dtype=np.uint32).reshape(-1, 4)
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1, 2)
    out = np.zeros_like(counters)
    rc = env["lib"].wc_philox4x32(env["ctx"], env["_lib"].ptr(counters), env["_lib"].ptr(keys), len(counters), env["_lib"].ptr(out))
    assert rc == 0, env["lib"].wc_last_error()
    return out


def test_known_answers_from_the_device_function(env):
    got = device_words(env, [k[0] for k in KNOWN], [k[1] for k in KNOWN])
    assert [" ".join("%08x" % w for w in row) for row in got] == [k[2] for k in KNOWN]
    rng = np.random.RandomState(5)
    counters = rng.randint(0, 2 ** 32, size=(4096, 4), dtype=np.uint64).astype(np.uint32)
    keys = rng.randint(0, 2 ** 32, size=(4096, 2), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(device_words(env, counters, keys), dr.philox(counters, keys))


# --------------------------------------------------------------------------------------------- k_thin ----
def thin_dev(env, base, sizes, keep, seed):
    """wc_thin_counts_dev; (rc, the output [n_keep, n_base, n_total], the guard row)."""
    torch, lib = env["torch"], env["lib"]
    keep = np.ascontiguousarray(keep, dtype=np.int32)
    n = len(keep) * base.size
    room = torch.full((n + base.shape[1],), FILL, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(np.array(base, dtype=np.int32)).cuda()
    rc = lib.wc_thin_counts_dev(env["ctx"], None, src.data_ptr(), base.shape[0], env["_lib"].ptr(sizes), len(sizes), env["_lib"].ptr(keep),
                                len(keep), seed, room.data_ptr())
    torch.cuda.synchronize()
    host = room.cpu().numpy()
    return rc, host[:n].reshape((len(keep),) + base.shape), host[n:]


@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("n_keep, n_base", [(1, 1), (2, 3), (8, 3), (8, 1)])
def test_thin_host_and_device_forms(env, n_keep, n_base, r):
    assert env["lib"].wc_thin_wave_cutoff() == dc.CUTOFF
    base, sizes, keep = dc.thin_base(n_base, r), dc.thin_sizes(r), dc.KEEPS[n_keep]
    want = dc.thin_want(n_base, r, n_keep, 1)
    got = env["se"].thinCounts(base, sizes, keep, seed=1)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    rc, dev, guard = thin_dev(env, base, sizes, keep, 1)
    assert rc == 0, env["lib"].wc_last_error()
    assert np.array_equal(dev, want) and (guard == FILL).all()
    # what the rule promises, on what the device gave
    negative = base < 0
    assert negative.any() and all(np.array_equal(dev[k][negative], base[negative]) for k in range(n_keep))
    if 1000000 in keep:
        assert np.array_equal(dev[keep.index(1000000)], base)
    order = np.argsort(keep)
    assert all((dev[order[i]] <= dev[order[i + 1]]).all() for i in range(n_keep - 1))


def test_thin_seed_with_its_high_word_set(env):
    base, sizes, keep = dc.thin_base(3, 1), dc.thin_sizes(1), dc.KEEPS[2] + [500000]
    want = dr.thin(base, sizes, keep, dc.HIGH_SEED)
    low_only = dr.thin(base, sizes, keep, dc.HIGH_SEED & 0xFFFFFFFF)
    assert not np.array_equal(want, low_only)
    assert np.array_equal(env["se"].thinCounts(base, sizes, keep, seed=dc.HIGH_SEED), want)
    rc, dev, guard = thin_dev(env, base, sizes, keep, dc.HIGH_SEED)
    assert rc == 0 and np.array_equal(dev, want) and (guard == FILL).all()


def test_thin_same_bits_twice_and_after_a_shorter_call(env):
    base, sizes, keep = dc.thin_base(3, 2), dc.thin_sizes(2), dc.KEEPS[8]
    want = dc.thin_want(3, 2, 8, 1)
    first = env["se"].thinCounts(base, sizes, keep, seed=1)
    shorter = env["se"].thinCounts(base[:1], sizes, keep[:2], seed=1)
    again = env["se"].thinCounts(base, sizes, keep, seed=1)
    assert np.array_equal(first, want) and np.array_equal(again, want)
    assert np.array_equal(shorter, want[:2, :1])


def test_thin_a_bin_of_exactly_two_to_the_24_reads(env):
    base, sizes, keep, want = dc.tower_want()
    got = env["se"].thinCounts(base, sizes, keep, seed=1)
    assert np.array_equal(got, want)
    assert abs(int(got[0, 0, 1]) - 2 ** 23) < 6 * 2 ** 11          # (sd = sqrt(2^24 / 4) = 2^11)


def test_thin_refuses_a_bin_beyond_the_limit_by_name(env):
    base = dc.thin_base(3, 0).copy()
    base[2, 77] = dc.MAX_READS + 1
    base[2, 500] = 2 ** 31 - 1
    rc, dev, guard = thin_dev(env, base, dc.thin_sizes(0), [500000, 250000], 1)
    message = env["lib"].wc_last_error().decode()
    assert rc == env["_lib"].E_LIMIT and "base row 2" in message and "bin 77 " in message, message
    assert (dev == FILL).all() and (guard == FILL).all()
    with pytest.raises(env["_lib"].WisecondorHipError, match="base row 2, bin 77 ") as err:
        env["se"].thinCounts(base, dc.thin_sizes(0), [500000])
    assert err.value.code == env["_lib"].E_LIMIT


@pytest.mark.parametrize("keep, sizes, word", [
    ([], None, "0 depths"), ([5] * 9, None, "9 depths"), ([500000, 0], None, "depth 1 keeps 0 ppm"),
    ([1000001], None, "depth 0 keeps 1000001 ppm"), ([5], [7, -1, 1015], "chromosome 2 has -1 bins"), ([5], [0, 0, 0], "a row without bins"),
])
def test_thin_refusals_name_the_argument_and_leave_the_output(env, keep, sizes, word):
    base = dc.thin_base(1, 0)
    sizes = dc.thin_sizes(0) if sizes is None else np.array(sizes, dtype=np.int64)
    torch, lib = env["torch"], env["lib"]
    room = torch.full((9 * base.size,), FILL, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(np.array(base, dtype=np.int32)).cuda()
    keep_room = np.array(keep + [7], dtype=np.int32)                 # (an empty list still has a pointer)
    rc = lib.wc_thin_counts_dev(env["ctx"], None, src.data_ptr(), 1, env["_lib"].ptr(sizes), len(sizes), env["_lib"].ptr(keep_room), len(keep), 1,
                                room.data_ptr())
    torch.cuda.synchronize()
    message = lib.wc_last_error().decode()
    assert rc == env["_lib"].E_ARG and word in message, message
    assert (room.cpu().numpy() == FILL).all()


# --------------------------------------------------------------------------------- the binomial spike ----
def spike_dev(env, base, sizes, plan, draw, seed, trial0, out_shift=0):
    """wc_spike_counts_ex_dev with the output `out_shift` elements behind a 16-byte address; (rc, rows, guard, saturated)."""
    torch, lib = env["torch"], env["lib"]
    n_total, n = int(sizes.sum()), len(plan)
    room = torch.full((out_shift + (n + 1) * n_total,), FILL, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(np.array(base, dtype=np.int32)).cuda()
    sat = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    plan = np.ascontiguousarray(plan, dtype=np.int32)
    rc = lib.wc_spike_counts_ex_dev(env["ctx"], None, src.data_ptr(), base.shape[0], env["_lib"].ptr(sizes), len(sizes), env["_lib"].ptr(plan), n,
                                    draw, seed, trial0, room.data_ptr() + 4 * out_shift, sat.data_ptr())
    torch.cuda.synchronize()
    host = room.cpu().numpy()
    return rc, host[out_shift:out_shift + n * n_total].reshape(n, n_total), np.concatenate([host[:out_shift], host[out_shift + n * n_total:]]), \
        int(sat.item())


@pytest.mark.parametrize("r", range(4))
@pytest.mark.parametrize("n_base", [1, 3])
def test_binomial_spike_host_and_device_forms(env, n_base, r):
    base, sizes, plan = dc.spike_base(n_base, r), dc.spike_sizes(r), dc.spike_plan(n_base, r)
    want, want_saturated = dc.spike_want(n_base, r, 1, 0)
    assert set(plan[:, 4].tolist()) == set(dc.SPIKE_PPM + [0]) and want_saturated == 1
    got, saturated = env["se"].spikeCounts(base, sizes, plan, draw=True, seed=1)
    assert got.dtype == np.int32 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert saturated == want_saturated
    for out_shift in range(4):
        rc, dev, guard, saturated = spike_dev(env, base, sizes, plan, 1, 1, 0, out_shift)
        assert rc == 0, env["lib"].wc_last_error()
        assert np.array_equal(dev, want), (out_shift, np.argwhere(dev != want)[:5])
        assert (guard == FILL).all() and saturated == want_saturated
    # a whole multiple of 1 000 000 ppm draws nothing: the deterministic rule's bits; the loss of everything is 0
    fixed = np.isin(plan[:, 4], [2000000, -1000000, 100000000, 0])
    assert np.array_equal(got[fixed], sr.spike(base, sizes, plan[fixed])[0])
    # a weak effect is no constant any more: the 300-bin span at 2.5 % adds more than two values
    weak = [i for i, row in enumerate(plan.tolist()) if row[3] == 300 and row[4] == 25000][0]
    added = (got[weak].astype(np.int64) - base[plan[weak, 0]])[9 + 100:9 + 400]
    assert len(set(added.tolist())) > 4 and abs(added.mean() - 7.5) < 6 * np.sqrt(7.5 / 300)


def test_binomial_spike_trial0_and_a_plan_cut_in_two(env):
    base, sizes, plan = dc.spike_base(3, 1), dc.spike_sizes(1), dc.spike_plan(3, 1)
    whole, _ = dc.spike_want(3, 1, dc.HIGH_SEED, 0)
    moved, _ = dc.spike_want(3, 1, dc.HIGH_SEED, 7)
    assert not np.array_equal(whole, moved)
    assert np.array_equal(env["se"].spikeCounts(base, sizes, plan, draw=True, seed=dc.HIGH_SEED, trial0=7)[0], moved)
    cut = 31
    first, _ = env["se"].spikeCounts(base, sizes, plan[:cut], draw=True, seed=dc.HIGH_SEED, trial0=0)
    second, _ = env["se"].spikeCounts(base, sizes, plan[cut:], draw=True, seed=dc.HIGH_SEED, trial0=cut)
    assert np.array_equal(np.concatenate([first, second]), whole)
    rc, dev, guard, _ = spike_dev(env, base, sizes, plan[cut:], 1, dc.HIGH_SEED, cut)
    assert rc == 0 and np.array_equal(dev, whole[cut:]) and (guard == FILL).all()


def test_draw_zero_through_the_ex_names_equals_the_first_names(env):
    for r in (0, 3):
        base, sizes, plan = dc.spike_base(3, r), dc.spike_sizes(r), dc.spike_plan(3, r)
        want, want_saturated = sr.spike(base, sizes, plan)
        old, old_saturated = env["se"].spikeCounts(base, sizes, plan)
        assert np.array_equal(old, want) and old_saturated == want_saturated
        for seed, trial0 in ((1, 0), (dc.HIGH_SEED, 7)):
            rc, dev, guard, saturated = spike_dev(env, base, sizes, plan, 0, seed, trial0, out_shift=r)
            assert rc == 0 and np.array_equal(dev, old) and (guard == FILL).all() and saturated == old_saturated
            out = np.full(old.shape, FILL, dtype=np.int32)
            sat = np.zeros(1, dtype=np.int64)
            rc = env["lib"].wc_spike_counts_ex(env["ctx"], env["_lib"].ptr(base), 3, env["_lib"].ptr(sizes), len(sizes), env["_lib"].ptr(plan),
                                               len(plan), 0, seed, trial0, env["_lib"].ptr(out), env["_lib"].ptr(sat))
            assert rc == 0 and np.array_equal(out, old) and int(sat[0]) == old_saturated


@pytest.mark.parametrize("draw, trial0, word", [(2, 0, "draw = 2"), (-1, 0, "draw = -1"), (1, -1, "trial0 = -1"), (1, 2 ** 32, "trial0 = 4294967296")])
def test_binomial_spike_refusals(env, draw, trial0, word):
    base, sizes, plan = dc.spike_base(1, 0), dc.spike_sizes(0), dc.spike_plan(1, 0)[:4]
    rc, dev, guard, saturated = spike_dev(env, base, sizes, plan, draw, 1, trial0)
    message = env["lib"].wc_last_error().decode()
    assert rc == env["_lib"].E_ARG and word in message, message
    assert (dev == FILL).all() and (guard == FILL).all() and saturated == -7
