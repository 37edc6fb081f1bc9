"""Jobs for the call-sequence tests (a helper module, not a conftest): one job per family of public entry points, each
in a SMALL and a LARGE shape, each a function of a context alone.

A wc_ctx holds about 130 grow-only workspaces, one pinned host block, side streams, a captured hipGraph and host-side
caches that describe device contents; whole families of entry points share them.  The suite's other files run on the
one context of _lib.context() in one fixed order.  Here a job is run on whatever context the caller hands it, after
whatever the caller ran there before, and must return the bits it returns on a context of its own (baseline()).

A job's run(ctx, shape) returns dict[str, np.ndarray | bytes]; same() compares two of them by bits (NaN payloads
included).  A job reaches the context through Reference(..., ctx=ctx) or a wrapper's ctx= argument where there is one,
otherwise through on_context(), which swaps the per-device context of _lib for the duration of the call -- test-side
only.  The shapes are the smallest that take the path in question; demand(shape) gives, by the size formulas of the
sources, what the shape asks of the workspaces the job uses (tests/test_sequence_cases_cpu.py holds LARGE > SMALL).
Each job's baseline is anchored once against the family's independent reference in tests/test_call_sequences_gpu.py.
"""
import contextlib
import functools
import os
import tempfile

import numpy as np

SMALL, LARGE = "small", "large"
SHAPES = (SMALL, LARGE)
KEYS24 = [str(c) for c in range(1, 23)] + ["X", "Y"]


# ------------------------------------------------------------------------------------------ plumbing ----
@contextlib.contextmanager
def on_context(ctx, device=0):
    """The wrappers without a ctx argument use _lib.context(device): hand them `ctx` instead, and put back what was."""
    from wisecondor_amd import _lib
    missing = object()
    old = _lib._contexts.get(device, missing)
    _lib._contexts[device] = ctx
    try:
        yield ctx
    finally:
        if old is missing:
            del _lib._contexts[device]
        else:
            _lib._contexts[device] = old


@contextlib.contextmanager
def environ(**values):
    """Environment switches of the library for the duration of a call (None: unset)."""
    old = {k: os.environ.get(k) for k in values}
    try:
        for k, v in values.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def epoch():
    from wisecondor_amd import _lib
    return int(_lib.load().wc_realloc_epoch())


def _bits(value):
    if isinstance(value, (bytes, bytearray)):
        return ("bytes", None, bytes(value))
    a = np.ascontiguousarray(value)
    return (str(a.dtype), a.shape, a.tobytes())


def same(got, want):
    """None, or what differs first: keys, then per key the dtype, the shape and the bytes."""
    if sorted(got) != sorted(want):
        return "keys %s, expected %s" % (sorted(got), sorted(want))
    for key in sorted(want):
        g, w = _bits(got[key]), _bits(want[key])
        if g[:2] != w[:2]:
            return "%s: %s %s, expected %s %s" % (key, g[0], g[1], w[0], w[1])
        if g[2] != w[2]:
            a, b = np.frombuffer(g[2], dtype=np.uint8), np.frombuffer(w[2], dtype=np.uint8)
            if len(a) != len(b):
                return "%s: %d bytes, expected %d" % (key, len(a), len(b))
            at = int(np.flatnonzero(a != b)[0])
            return "%s: %d of %d bytes differ, the first at byte %d" % (key, int((a != b).sum()), len(a), at)
    return None


def _frozen(a):
    a.setflags(write=False)
    return a


# ------------------------------------------------------------------------------------------ 1 newref ----
NEWREF_SIZES = {SMALL: (120, 100, 80), LARGE: (400, 300, 200)}
NEWREF_SAMPLES, NEWREF_K = 40, 40


@functools.lru_cache(maxsize=None)
def newref_case(shape):
    sizes = np.array(NEWREF_SIZES[shape], dtype=np.int64)
    rng = np.random.RandomState(11 + len(shape))
    data = 1.0 + 0.02 * rng.standard_normal((int(sizes.sum()), NEWREF_SAMPLES))
    return _frozen(data), _frozen(sizes)


def run_newref(ctx, shape):
    from wisecondor_amd import wisetools as wt
    data, sizes = newref_case(shape)
    out = {}
    with on_context(ctx):
        for order, arr in (("F", np.asfortranarray(data)), ("C", np.ascontiguousarray(data))):
            idx, dst = wt.getReference(arr, sizes, np.cumsum(sizes), NEWREF_K, 1, 1)
            out["idx_" + order], out["dst_" + order] = idx, dst
    return out


def demand_newref(shape):
    b = sum(NEWREF_SIZES[shape])
    return {"corrected image": 8 * b * NEWREF_SAMPLES, "lists out": 12 * b * NEWREF_K, "padded rows": -(-b // 128) * 128}


# -------------------------------------------------------------------------------------------- 2 prep ----
PREP_CASES = {SMALL: (40, 700), LARGE: (100, 1025)}
PREP_COMPS = (1, 8)


def run_prep_one(ctx, shape, n_comp):
    import prep_cases as pc
    from wisecondor_amd import wisetools as wt
    counts, sizes = pc.make_case(*PREP_CASES[shape])
    with on_context(ctx):
        masked, bins, mask, corrected, comps, mean, mbins = wt.prepReference(None, pcacomp=n_comp, counts=counts, chrom_bins=sizes)
    return {"masked": np.array(masked), "mask": np.asarray(mask), "corrected": np.ascontiguousarray(corrected), "comps": comps,
            "mean": mean, "mbins": np.asarray(mbins, dtype=np.int64), "bins": np.asarray(bins, dtype=np.int64)}


def run_prep(ctx, shape):
    out = {}
    for n_comp in PREP_COMPS:
        out.update(("%s_%d" % (k, n_comp), v) for k, v in run_prep_one(ctx, shape, n_comp).items())
    return out


def demand_prep(shape):
    s, b = PREP_CASES[shape]
    total = b + max(2, int(round(b / 9.0)))
    return {"counts": 4 * s * total, "masked data": 8 * b * s, "gram and components": 8 * (s * s + 8 * s + 9 * b),
            "pinned components": 8 * max(PREP_COMPS) * b}


# ----------------------------------------------------------------------- 3, 4 the test path's layout ----
TEST_SIZES = (130, 120, 115, 105, 100, 95, 90, 85, 80, 75, 75, 70, 60, 55, 50, 45, 45, 40, 30, 30, 25, 25)
TEST_THR = 5.0
TEST_SAMPLES = {SMALL: 12, LARGE: 40}           # 40 samples: padded to 48 for the z-score tiles
LAT_SAMPLES = {SMALL: 1, LARGE: 3}


@functools.lru_cache(maxsize=None)
def tp_layout():
    """The layout of test_testpath_gpu's late-repeats case at half the chromosome lengths (1 545 bins, nothing masked, 30
    reference samples, k = 40, three components).  The neighbour lists come from the CPU oracle, so the layout does not
    depend on any context.  A dict as wo.test_sample takes it."""
    from oracle import wc_oracle as wo
    rng = np.random.RandomState(77)
    sizes = np.array(TEST_SIZES, dtype=np.int64)
    total = int(sizes.sum())
    corrected = np.asfortranarray(1.0 + 0.02 * rng.standard_normal((total, 30)))
    idx, dst = wo.get_reference(corrected, sizes, np.cumsum(sizes), 40, 1, 1, fast=True)
    comps = np.linalg.qr(rng.standard_normal((total, 3)))[0].T
    mean = np.full(total, 1.0 / total) * (1 + 0.01 * rng.standard_normal(total))
    out = dict(binsize=np.float64(1e6), indexes=np.ascontiguousarray(idx, dtype=np.int32), distances=np.ascontiguousarray(dst),
               chromosome_sizes=sizes, mask=np.ones(total, dtype=bool), masked_sizes=sizes, pca_mean=mean,
               pca_components=np.ascontiguousarray(comps))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tp_samples():
    """48 sample dicts: scattered loud bins (repeats 3 and 4 still flag some) and one planted gain or loss each."""
    sizes = np.array(TEST_SIZES, dtype=np.int64)
    total = int(sizes.sum())
    offs = np.concatenate([[0], np.cumsum(sizes)])
    rng = np.random.RandomState(5)
    out = []
    for i in range(48):
        lam = np.full(total, 2500.0) * (1 + 0.02 * rng.standard_normal(total)).clip(0.5)
        lam[rng.rand(total) < 0.1] *= 1.15
        c = i % 7
        lam[offs[c] + 10 + i % 13:offs[c] + 40 + i % 13] *= 1.3 if i % 2 else 0.75
        counts = rng.poisson(lam).astype(np.int32)
        out.append({str(k + 1): _frozen(counts[offs[k]:offs[k + 1]].copy()) for k in range(22)})
    return tuple(out)


_references = {}


def reference_on(ctx, which="test"):
    """The wisetools.Reference of a layout in `ctx` -- "test": tp_layout(), "spike": the short layout of call_cases with
    the first base sample's mean (spike_cases) -- made at the first use and kept until close_references(ctx): creating
    and destroying a reference allocates, the calls on it must not."""
    from wisecondor_amd import wisetools as wt
    if (ctx, which) not in _references:
        if which == "test":
            lay = tp_layout()
            ref = wt.Reference(lay["indexes"], lay["distances"], lay["chromosome_sizes"], lay["masked_sizes"], lay["mask"],
                               lay["pca_mean"], lay["pca_components"], binsize=float(lay["binsize"]), ctx=ctx)
        else:
            import call_cases as cc
            import spike_cases as sc
            lay = sc.lay()
            ref = wt.Reference(lay["idx"], lay["dst"], lay["sizes"], lay["msizes"], lay["mask"], sc.base_samples()[0]["pca_mean"],
                               lay["pca_components"], binsize=cc.BINSIZE, ctx=ctx)
        _references[(ctx, which)] = ref
    return _references[(ctx, which)]


def close_references(ctx):
    """Before the context is destroyed, or to have the next job make its reference anew."""
    for key in [k for k in _references if k[0] == ctx]:
        _references.pop(key).close()


@contextlib.contextmanager
def context():
    """A context of its own, destroyed (with the references made in it) on the way out."""
    from wisecondor_amd import _lib
    ctx = _lib.new_context(0)
    try:
        yield ctx
    finally:
        close_references(ctx)
        _lib.destroy_context(ctx)


def batch_outputs(outs):
    """The list of wisetools.test_batch as arrays: every member of every sample."""
    calls = [np.asarray(o["results_calls"], dtype=np.float64).reshape(-1, 5) for o in outs]
    return {"z": np.stack([np.concatenate(o["results_z"]) for o in outs]), "r": np.stack([np.concatenate(o["results_r"]) for o in outs]),
            "cwz": np.stack([np.asarray(o["results_cwz"], dtype=np.float64) for o in outs]), "calls": np.concatenate(calls),
            "n_calls": np.array([len(c) for c in calls], dtype=np.int64), "asdef": np.array([o["asdef"] for o in outs], dtype=np.float64)}


def tp_call(reference, first, count, mode=None):
    """One wisetools.test_batch of samples [first, first + count) under WC_TEST_LATENCY_MODE = mode (None: automatic)."""
    from wisecondor_amd import wisetools as wt
    with environ(WC_TEST_LATENCY_MODE=mode):
        return batch_outputs(wt.test_batch(reference, list(tp_samples()[first:first + count]), TEST_THR))


def run_test_general(ctx, shape):
    return tp_call(reference_on(ctx), 0, TEST_SAMPLES[shape])


def run_test_latency(ctx, shape):
    """Three calls -- an eager one that sizes the workspaces, the capture, a replay -- and the third call's outputs."""
    return [tp_call(reference_on(ctx), 20, LAT_SAMPLES[shape]) for _ in range(3)][-1]


def _demand_test(n):
    total = sum(TEST_SIZES)
    return {"counts": 4 * n * total, "z and r": 16 * n * total, "calls": 40 * 256 * n}


def demand_test_general(shape):
    n = TEST_SAMPLES[shape]
    return dict(_demand_test(n), **{"padded samples": -(-n // 16) * 16})


def demand_test_latency(shape):
    return _demand_test(LAT_SAMPLES[shape])


# ------------------------------------------------------------------- 5 the small test-path entries ----
SMALL_REGIONS = {SMALL: (40, 150, 7), LARGE: (300, 700, 40, 150)}
SMALL_ROWS = {SMALL: 3, LARGE: 33}
SMALL_APPLY = {SMALL: (3, 2047), LARGE: (5, 8193)}          # (components, bins) of prep_cases.apply_case


@functools.lru_cache(maxsize=None)
def small_case(shape):
    rng = np.random.RandomState(11 + len(shape))
    regions = []
    for n in SMALL_REGIONS[shape]:
        z = rng.standard_normal(n)
        z[n // 3:n // 3 + max(1, n // 5)] += 2.5
        regions.append(_frozen(z))
    rows = SMALL_ROWS[shape]
    lay = tp_layout()
    total = int(lay["masked_sizes"].sum())
    sd = rng.gamma(3.0, 0.1, size=(rows, 300 if shape == SMALL else 3000))
    sd[rng.rand(*sd.shape) < 0.05] = np.nan
    data = (1.0 + 0.02 * rng.standard_normal((rows, total)))
    data[:, 200:230] *= 1.3
    return dict(regions=tuple(regions), sd=_frozen(sd), data=_frozen(data))


def run_small(ctx, shape):
    import prep_cases as pc
    from wisecondor_amd import wisetools as wt
    case, lay = small_case(shape), tp_layout()
    out = {}
    with on_context(ctx):
        whole, segs = wt.stouffer_segments(list(case["regions"]), 3.0, 3)
        out["whole"] = whole
        out["segs"] = np.array([[r, v, x, y] for r, rows in enumerate(segs) for v, (x, y) in rows], dtype=np.float64).reshape(-1, 4)
        cutoff, mask = wt.getOptimalCutoff(lay["distances"], 3)
        out["cutoff"], out["cutoff_mask"] = np.array([cutoff]), mask
        out["sd_avg"] = np.asarray(wt.stdDevAvg(case["sd"]))
        ms = lay["masked_sizes"]
        z, r, n, sd = wt.repeatTest(case["data"], lay["indexes"], lay["distances"], ms, np.cumsum(ms), cutoff, 4.0, 3,
                                    reference=reference_on(ctx))
        out["rep_z"], out["rep_r"], out["rep_n"], out["rep_sd"] = z, r, n, sd
        x, mean, comps = pc.apply_case(*SMALL_APPLY[shape])
        out["pca"] = wt.applyPCA(x[:SMALL_ROWS[shape]], mean, comps)
    return out


def demand_small(shape):
    return {"regions": 8 * sum(SMALL_REGIONS[shape]), "longest region": max(SMALL_REGIONS[shape]),
            "repeat rows": 8 * SMALL_ROWS[shape] * sum(TEST_SIZES), "sd rows": 8 * SMALL_ROWS[shape] * (300 if shape == SMALL else 3000),
            "pca rows": 8 * SMALL_ROWS[shape] * SMALL_APPLY[shape][1]}


# -------------------------------------------------------------------------------------------- 6 eigh ----
EIGH = {SMALL: (100, 3), LARGE: (300, 8)}


@functools.lru_cache(maxsize=None)
def eigh_case(shape):
    n, _ = EIGH[shape]
    a = np.random.default_rng(n).standard_normal((n, n))
    return _frozen(a + a.T)


def run_eigh(ctx, shape):
    from wisecondor_amd import wisetools as wt
    with on_context(ctx):
        vals, vecs = wt.sym_eigh_leading(eigh_case(shape), EIGH[shape][1])
    return {"vals": vals, "vecs": vecs}


def demand_eigh(shape):
    n, k = EIGH[shape]
    return {"working copy": 8 * n * n, "vectors": 8 * n * k}


# ----------------------------------------------------------------------------------------- 7 convert ----
CONVERT_READS = {SMALL: 150, LARGE: 600}        # per reference, 25 references
CONVERT_BINSIZE = 50000.0
_tmp = None


def _tmp_dir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="wc_sequence_cases_")
    return _tmp.name


@functools.lru_cache(maxsize=None)
def convert_case(shape):
    """(names, lengths, per-reference sorted positions, qualities) of 25 references (chrM is not binned) with towers of
    reads at one position and qualities of 0 among them."""
    rng = np.random.RandomState(40 + len(shape))
    refs = [("chr%s" % k, 2000000 + 100000 * i) for i, k in enumerate(KEYS24)] + [("chrM", 16571)]
    pos, mapq = [], []
    for r, (_, length) in enumerate(refs):
        n = CONVERT_READS[shape] + 10 * r
        p = np.concatenate([rng.randint(0, length, n), np.full(6, length // 2), length // 3 + np.arange(5)])
        pos.append(_frozen(np.sort(p).astype(np.int64)))
        mapq.append(_frozen(np.where(rng.rand(len(p)) < 0.1, 0, 60).astype(np.int64)))
    return [n for n, _ in refs], [l for _, l in refs], tuple(pos), tuple(mapq)


@functools.lru_cache(maxsize=None)
def convert_bam(shape):
    import bam_writer as bw
    names, lengths, pos, mapq = convert_case(shape)
    path = os.path.join(_tmp_dir(), "%s.bam" % shape)
    bw.write_bam(path, list(zip(names, lengths)), bw.records_of(list(range(len(names))), pos, mapq, unplaced=7), seed=40)
    return path


def sample_arrays(tag, sample, info):
    out = {"%s_%s" % (tag, k): (np.zeros(0, dtype=np.int32) if sample.get(k) is None else np.asarray(sample[k], dtype=np.int32))
           for k in KEYS24}
    out[tag + "_info"] = np.array([int(info[k]) for k in sorted(info)], dtype=np.int64)
    return out


def run_convert(ctx, shape):
    from wisecondor_amd import wisetools as wt
    names, lengths, pos, mapq = convert_case(shape)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
    out = {}
    with on_context(ctx):
        sample, info = wt.convertReads(names, lengths, offsets, np.concatenate(pos).astype(np.int32),
                                       np.concatenate(mapq).astype(np.uint8), CONVERT_BINSIZE, 4, 4)
        out.update(sample_arrays("reads", sample, info))
        with wt.BamReadsDevice(convert_bam(shape)) as bam:
            sample, info = wt.convertBamReads(bam, CONVERT_BINSIZE, 4, 4)
        out.update(sample_arrays("bam", sample, info))
    return out


def demand_convert(shape):
    reads = sum(CONVERT_READS[shape] + 10 * r + 11 for r in range(25))
    return {"positions": 4 * reads, "qualities": reads, "file bytes": os.path.getsize(convert_bam(shape))}


# ----------------------------------------------------------------------------------------- 8 deflate ----
DEFLATE = {SMALL: (3, 5000), LARGE: (9, 70001)}          # rows, bytes per row (70 001: more than one 64 KiB block)


@functools.lru_cache(maxsize=None)
def deflate_case(shape):
    n, width = DEFLATE[shape]
    rng = np.random.RandomState(width)
    rows = rng.randint(0, 256, size=(n, width)).astype(np.uint8)
    rows[:, width // 4:width // 2] = rows[:, :width // 4][:, :width // 2 - width // 4]       # something to match
    rows[0, :] = 7                                                                          # one long run
    return _frozen(rows)


def run_deflate(ctx, shape):
    from wisecondor_amd import wisetools as wt
    rows = deflate_case(shape)
    streams, lengths, crcs = wt.deflateRows(rows, ctx=ctx)
    out = {"lengths": lengths, "crcs": crcs}
    for i in range(len(rows)):
        out["stream_%d" % i] = streams[i, :lengths[i]].tobytes()
    with on_context(ctx):
        out["adler"] = wt.adler32Rows(rows)
    return out


def demand_deflate(shape):
    n, width = DEFLATE[shape]
    return {"rows": n * width, "blocks per row": -(-width // 65536)}


# ------------------------------------------------------------------------------------------ 9 export ----
EXPORT_RESULTS = {SMALL: 2, LARGE: 9}


@functools.lru_cache(maxsize=None)
def export_case(shape):
    import json_cases
    return tuple(json_cases.synthetic_result(40 + i) for i in range(EXPORT_RESULTS[shape]))


def run_export(ctx, shape):
    import json_cases
    from wisecondor_amd import wisetools as wt
    results = list(export_case(shape))
    rows = json_cases.dense([r["results_z"] for r in results])
    out = {}
    for i, text in enumerate(wt.jsonRows(rows, json_cases.SIZES, ctx=ctx)):
        out["json_row_%d" % i] = text
    for i, data in enumerate(wt.export_json_batch(results, gz=True, ctx=ctx)):
        out["json_gz_%d" % i] = bytes(data)
    texts, dropped = wt.bedgraphRows(rows, json_cases.SIZES, 250000, ctx=ctx)
    for i, text in enumerate(texts):
        out["bedgraph_row_%d" % i] = text
    out["bedgraph_dropped"] = np.asarray(dropped, dtype=np.int64)
    for i, files in enumerate(wt.export_tracks_batch(results, gz=True, ctx=ctx)):
        for k, data in enumerate(files):
            out["track_%d_%d" % (i, k)] = bytes(data)
    return out


def demand_export(shape):
    import json_cases
    return {"rows": 8 * 2 * EXPORT_RESULTS[shape] * sum(json_cases.SIZES), "text rows": 2 * EXPORT_RESULTS[shape]}


# ---------------------------------------------------------------------------------------- 10 plot ----
PLOT = {SMALL: ("five_c3", 1, 50), LARGE: ("all22_c2", 3, 100)}          # case of plot_cases, samples, dpi (4 x 3 inches)


@functools.lru_cache(maxsize=None)
def plot_case(shape):
    import plot_cases
    name, n, dpi = PLOT[shape]
    case = {c["name"]: c for c in plot_cases.cases()}[name]
    steps = (1, 0, 2)[:n]
    results = []
    for i, step in enumerate(steps):
        calls = case["calls"] if step == 1 else (np.array([]) if step == 0 else np.asarray(case["calls"])[::step])
        results.append(dict(results_z=plot_cases.zscores(6 * i), results_calls=calls, threshold_z=case["threshold"], binsize=case["binsize"]))
    return case, tuple(results), tuple("s%d_%s" % (i, "x" * i) for i in range(n)), dpi


def run_plot(ctx, shape):
    from wisecondor_amd import wisetools as wt
    case, results, names, dpi = plot_case(shape)
    with on_context(ctx):
        entries, counts, status = wt.plotList([r["results_z"] for r in results], [r["results_calls"] for r in results], case["threshold"],
                                              case["chromosomes"], case["mineffect"])
    details = {}
    pngs = wt.plot_batch(list(results), list(names), chromosomes=case["chromosomes"], columns=case["columns"], size=(4.0, 3.0),
                         mineffect=case["mineffect"], dpi=dpi, ctx=ctx, details=details)
    out = {"entries": entries, "counts": counts, "status": np.array([status]), "scanlines": details["scanlines"]}
    for i, png in enumerate(pngs):
        out["png_%d" % i] = bytes(png)
    return out


def demand_plot(shape):
    _, n, dpi = PLOT[shape]
    case = plot_case(shape)[0]
    return {"images": n * (4 * dpi) * (1 + 3 * 3 * dpi), "lists": n * len(case["chromosomes"])}


# ----------------------------------------------------------------------------------------- 11 pdf ----
PDF_PAGES = {SMALL: 2, LARGE: 66}           # 66 pages x 22 panels x 4 bytes of counts: more than prep's 700 x 8 bytes pinned
PDF_CASE = {SMALL: "five_c2", LARGE: "all22_c2"}


@functools.lru_cache(maxsize=None)
def pdf_case(shape):
    import plot_cases
    case = {c["name"]: c for c in plot_cases.cases()}[PDF_CASE[shape]]
    results = []
    for i in range(PDF_PAGES[shape]):
        step = (1, 0, 2, 3)[i % 4]
        calls = case["calls"] if step == 1 else (np.array([]) if step == 0 else np.asarray(case["calls"])[::step])
        results.append(dict(results_z=plot_cases.zscores(6 * (i % 5)), results_calls=calls, threshold_z=case["threshold"],
                            binsize=case["binsize"]))
    return case, tuple(results), tuple("p%d" % i for i in range(len(results)))


def run_pdf(ctx, shape):
    from wisecondor_amd import wisetools as wt
    case, results, names = pdf_case(shape)
    details = {}
    files = wt.plot_pdf_batch(list(results), list(names), chromosomes=case["chromosomes"], columns=case["columns"], size=(4.0, 3.0),
                              mineffect=case["mineffect"], ctx=ctx, details=details)
    out = {}
    for i, data in enumerate(files):
        out["pdf_%d" % i] = bytes(data)
        out["content_%d" % i] = details["content"][i]
    return out


def demand_pdf(shape):
    case = pdf_case(shape)[0]
    return {"pinned counts": 4 * PDF_PAGES[shape] * len(case["chromosomes"]), "pages": PDF_PAGES[shape]}


# --------------------------------------------------------------------------------- 12 sensitivity ----
SENS_ROWS = {SMALL: (0, 4, 13, 14), LARGE: tuple(range(20))}         # rows of spike_cases.designed_plan()
SENS_KEEP = {SMALL: (500000,), LARGE: (1000000, 900000, 250000, 1000)}
SENS_SEED = 0x9E3779B97F4A7C15


def sens_plan(shape):
    import spike_cases as sc
    return np.ascontiguousarray(sc.designed_plan()[list(SENS_ROWS[shape])])


def sens_calls(shape):
    """Call rows for scoreTrials: every trial's own span as one call, and a miss beside it."""
    plan = sens_plan(shape)
    calls = np.zeros((len(plan), 4, 5))
    n_calls = np.zeros(len(plan), dtype=np.int32)
    for i, (_, chrom, first, bins, ppm) in enumerate(plan.tolist()):
        if ppm:
            calls[i, 0] = (chrom, first, first + bins - 1, 6.5 if ppm > 0 else -6.5, ppm / 1e6)
            calls[i, 1] = (chrom % 22 + 1, 0, 2, 5.5, 0.01)
            n_calls[i] = 2
    return calls, n_calls


def run_sensitivity(ctx, shape):
    import call_cases as cc
    import spike_cases as sc
    from wisecondor_amd import wisetools as wt
    lay, base, plan = sc.lay(), sc.base_counts(), sens_plan(shape)
    out = {}
    with on_context(ctx):
        out["thinned"] = wt.thinCounts(base, lay["sizes"], list(SENS_KEEP[shape]), seed=SENS_SEED)
        out["spiked"], saturated = wt.spikeCounts(base, lay["sizes"], plan)
        out["drawn"], saturated_drawn = wt.spikeCounts(base, lay["sizes"], plan, draw=True, seed=SENS_SEED, trial0=3)
        out["saturated"] = np.array([saturated, saturated_drawn], dtype=np.int64)
        calls, n_calls = sens_calls(shape)
        out["score_i"], out["score_f"] = wt.scoreTrials(plan, calls, n_calls)
    rec_i, rec_f, kept = wt.sensitivity_batch(reference_on(ctx, "spike"), [s["counts"] for s in sc.base_samples()], plan, cc.THR,
                                              minrefbins=cc.MINREF, repeats=cc.REPEATS, keep_calls=True)
    out["rec_i"], out["rec_f"] = rec_i, rec_f
    out["kept_calls"] = np.concatenate([np.asarray(k, dtype=np.float64).reshape(-1, 5) for k in kept])
    out["kept_n"] = np.array([len(k) for k in kept], dtype=np.int64)
    return out


def demand_sensitivity(shape):
    total = 994 + 32
    return {"spiked rows": 4 * len(SENS_ROWS[shape]) * total, "thinned rows": 4 * 2 * len(SENS_KEEP[shape]) * total,
            "plan rows": 20 * len(SENS_ROWS[shape])}


# ------------------------------------------------------------------------------------ 13 crossval ----
CROSSVAL = {SMALL: (5, (9, 4, 0, 12)), LARGE: (70, (60, 58, 52, 50, 47, 45, 42, 40, 38, 36, 130))}
CROSSVAL_LENGTHS = (1, 2, 5)


@functools.lru_cache(maxsize=None)
def crossval_case(shape):
    import crossval_cases
    n, sizes = CROSSVAL[shape]
    return crossval_cases.random_case(21 + n, n, list(sizes), max_calls=3, lengths=CROSSVAL_LENGTHS)


def run_crossval(ctx, shape):
    from wisecondor_amd import crossval
    case = crossval_case(shape)
    with on_context(ctx):
        return dict(crossval.crossvalStats(case["Z"], case["sizes"], case["thr"], case["asdef"], case["calls"], case["n_calls"],
                                           chromosomes=case["sel"], windows=case["lengths"]))


def demand_crossval(shape):
    n, sizes = CROSSVAL[shape]
    return {"Z": 8 * n * sum(sizes), "prefix sums": 8 * n * (sum(sizes) + len(sizes)), "rows": 4 * n * len(sizes)}


# ------------------------------------------------------------------------------------- the registry ----
class Job(object):
    def __init__(self, name, run, demand):
        self.name, self.run, self.demand = name, run, demand

    def __repr__(self):
        return self.name


JOBS = [Job("newref", run_newref, demand_newref), Job("prep", run_prep, demand_prep),
        Job("test_general", run_test_general, demand_test_general), Job("test_latency", run_test_latency, demand_test_latency),
        Job("small_entries", run_small, demand_small), Job("eigh", run_eigh, demand_eigh), Job("convert", run_convert, demand_convert),
        Job("deflate", run_deflate, demand_deflate), Job("export", run_export, demand_export), Job("plot", run_plot, demand_plot),
        Job("pdf", run_pdf, demand_pdf), Job("sensitivity", run_sensitivity, demand_sensitivity),
        Job("crossval", run_crossval, demand_crossval)]
BY_NAME = {job.name: job for job in JOBS}
NAMES = [job.name for job in JOBS]

_baselines = {}


def fresh(fn, *args):
    """fn(ctx, *args) on a context created for it and destroyed after."""
    with context() as ctx:
        return fn(ctx, *args)


def baseline(name, shape):
    """The job's outputs on a context of its own, computed once and shared: read-only."""
    key = (name, shape)
    if key not in _baselines:
        out = fresh(BY_NAME[name].run, shape)
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _baselines[key] = out
    return _baselines[key]


def walk_steps(seed, n_steps=40):
    """The seeded walk of a seed: n_steps (job name, shape) pairs."""
    rng = np.random.RandomState(1000 + seed)
    return [(NAMES[rng.randint(len(NAMES))], SHAPES[rng.randint(2)]) for _ in range(n_steps)]
