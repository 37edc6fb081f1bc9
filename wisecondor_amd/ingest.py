"""Sample-file ingest and result-file output for many samples.

The upstream tools read one converted sample after the other with np.load inside the
driver loop (wisecondor.py:75-80, 193-196) and `test` handles one file per process.
Once the GPU side takes a fraction of a millisecond per sample, decoding the .npz
members (zip inflate + unpickle of the chromosome dict) and encoding the result files
is the ceiling -- and in Python both hold the GIL for most of their time.  So both run in
the library's C++ thread pools (csrc/npzio.cpp: zip, a small pickle machine, zlib), batches are
double buffered, and the dense count rows are staged in pinned host memory for the copy
engine.  Nothing numeric happens here.
"""
import argparse
import collections
import concurrent.futures
import ctypes
import os
import pickle
import time

import numpy as np

from . import _lib
from . import wisetools as wt

LoadedSamples = collections.namedtuple('LoadedSamples', 'samples binsizes')


def read_sample(path, to_binsize=None):
    """(chromosome -> int32[bins] dict at `to_binsize`, the file's own bin size)."""
    stored = np.load(path, allow_pickle=True, encoding='latin1')
    own = stored['arguments'].item()['binsize']
    return wt.scaleSample(stored['sample'].item(), own, to_binsize), own


def load_samples(paths, to_binsize=None, threads=8, verbose=False):
    """All samples of `paths`, decoded in a thread pool, in the given order."""
    began = time.time()
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, threads)) as pool:
        got = list(pool.map(lambda p: read_sample(p, to_binsize), paths))
    if verbose:
        for path, (_, own) in zip(paths, got):
            print('read %s (binsize %d)' % (path, int(own)))
        print('%d sample files in %.2f s' % (len(paths), time.time() - began))
    return LoadedSamples([g[0] for g in got], set(g[1] for g in got))


def _count_row(path, to_binsize, sizes, out_row):
    sample, _ = read_sample(path, to_binsize)
    out_row[:] = wt.samples_to_counts([sample], sizes)[0]


# ---------------------------------------------------------------- native I/O ----
def _c_strings(items):
    arr = (ctypes.c_char_p * len(items))()
    arr[:] = [os.fsencode(p) for p in items]
    return arr


def read_counts(paths, chrom_sizes, to_binsize, out_rows, threads=8, fallbacks=None):
    """Rows of `out_rows` (int32 [>= len(paths), sum(chrom_sizes)], C-contiguous rows) = the dense
    count vectors of the sample files, decoded by the library's C++ thread pool
    (wc_read_samples: zip inflate, the pickled chromosome dict, scaleSample, pad / truncate).
    A file the native reader does not understand is read with np.load instead -- same result,
    and np.load's own error if the file is broken.  Returns the files' own bin sizes; `fallbacks`
    (a list) collects the positions of the files that took the np.load path."""
    n = len(paths)
    sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
    assert out_rows.dtype == np.int32 and out_rows.shape[1] == int(sizes.sum()) and out_rows.strides[1] == 4
    own = np.zeros(n, dtype=np.float64)
    status = np.zeros(n, dtype=np.int32)
    if n == 0:
        return own
    _lib.check(_lib.load().wc_read_samples(_c_strings(paths), n, int(threads), _lib.ptr(sizes), len(sizes),
                                           float(to_binsize or 0.0), ctypes.c_void_p(out_rows.ctypes.data),
                                           out_rows.strides[0] // 4, _lib.ptr(own), _lib.ptr(status)))
    if fallbacks is not None:
        fallbacks.extend(int(i) for i in np.nonzero(status)[0])      # (tests: which files the native reader passed on)
    for i in np.nonzero(status)[0]:
        sample, size = read_sample(paths[i], to_binsize)      # raises what the reference would report
        out_rows[i, :] = wt.samples_to_counts([sample], sizes)[0]
        own[i] = size
    return own


def load_counts(paths, to_binsize=None, threads=8, verbose=False):
    """`newref`'s sample load as one dense matrix: (counts int32 [files, sum(chrom_bins)], chrom_bins[22],
    the set of the files' own bin sizes).  chrom_bins is the per-chromosome maximum over the samples
    (toNumpyArray, wisetools.py:243-250); two native passes over the files (lengths, then rows), np.load
    for any file the native reader passes on."""
    began = time.time()
    n = len(paths)
    lens = np.zeros((n, 22), dtype=np.int64)
    own = np.zeros(n, dtype=np.float64)
    status = np.zeros(n, dtype=np.int32)
    if n:
        _lib.check(_lib.load().wc_read_sample_lengths(_c_strings(paths), n, int(threads), 22, float(to_binsize or 0.0),
                                                      _lib.ptr(lens), _lib.ptr(own), _lib.ptr(status)))
    for i in np.nonzero(status)[0]:
        sample, size = read_sample(paths[i], to_binsize)
        lens[i] = [len(sample[str(c)]) for c in range(1, 23)]
        own[i] = size
    chrom_bins = [int(v) for v in lens.max(axis=0)] if n else [0] * 22
    counts = np.zeros((n, int(sum(chrom_bins))), dtype=np.int32)
    read_counts(paths, chrom_bins, to_binsize, counts, threads=threads)
    if verbose:
        for path, size in zip(paths, own):
            print('read %s (binsize %d)' % (path, int(size)))
        print('%d sample files in %.2f s' % (n, time.time() - began))
    return counts, chrom_bins, set(float(v) for v in own)


def _object_npy(obj):
    """Bytes of the .npy member np.savez writes for a Python object (a 0-d object array)."""
    header = b"{'descr': '|O', 'fortran_order': False, 'shape': (), }"
    pad = (64 - (10 + len(header) + 1) % 64) % 64
    header = header + b' ' * pad + b'\n'
    body = pickle.dumps(np.array(obj, dtype=object), protocol=3)
    return b'\x93NUMPY\x01\x00' + len(header).to_bytes(2, 'little') + header + body


def check_encoder(encoder, level):
    """'host' or 'gpu'; the GPU encoder is one strategy (run-length matches, a Huffman code per block: what the host
    writer does at level 1), not a zlib level, so it goes with -ziplevel 1 only."""
    if encoder not in ('host', 'gpu'):
        raise ValueError("encoder: 'host' or 'gpu', not %r" % (encoder,))
    if encoder == 'gpu' and int(level) != 1:
        raise ValueError('-encoder gpu writes run-length deflate, which is -ziplevel 1; -ziplevel %d (%s) is the host '
                         "encoder's" % (int(level), 'stored' if int(level) == 0 else 'zlib\'s string search'))
    return encoder


def pack_results(members, z, r, ctx=None):
    """results_z / results_r of a batch as ready-made zip members, on the device: the .npy images of the rows of the
    device tensors z and r (wt.ResultMembers), deflated row by row (wt.deflateRows).  Returns the six device tensors
    (z streams, lengths, crcs, r streams, lengths, crcs)."""
    return wt.deflateRows(members.image(z, ctx=ctx), ctx=ctx) + wt.deflateRows(members.image(r, ctx=ctx), ctx=ctx)


def _host_array(a):
    return a if isinstance(a, np.ndarray) else np.ascontiguousarray(a.detach().cpu().numpy())


def _native_write(entry, out_paths, per_file_args, runtime, binsize, threshold_z, big, cwz, calls, n_calls, asdef, threads,
                  level):
    """wc_write_test_results / wc_write_test_results_packed: `big` is what the entry takes for results_z / results_r."""
    n = len(out_paths)
    blobs = [_object_npy(vars(a) if not isinstance(a, dict) else a) for a in per_file_args]
    blob_ptrs = (ctypes.c_char_p * n)()
    blob_ptrs[:] = blobs
    lens = np.array([len(b) for b in blobs], dtype=np.int64)
    rt = _object_npy(runtime)
    status = np.zeros(n, dtype=np.int32)
    for a in (cwz, calls, asdef):
        assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS']
    assert n_calls.dtype == np.int32
    _lib.check(entry(
        n, int(threads), _c_strings(out_paths), blob_ptrs, _lib.ptr(lens), rt, len(rt), float(binsize),
        int(isinstance(binsize, (int, np.integer)) and not isinstance(binsize, bool)), float(threshold_z), *big, _lib.ptr(cwz),
        cwz.shape[1], _lib.ptr(calls), _lib.ptr(n_calls), calls.shape[1], _lib.ptr(asdef), int(level), _lib.ptr(status)))
    bad = np.nonzero(status)[0]
    if len(bad):
        raise IOError('could not write %d result file(s), first: %s' % (len(bad), out_paths[bad[0]]))


def write_packed(out_paths, per_file_args, runtime, binsize, threshold_z, member_bytes, packed, cwz, calls, n_calls, asdef,
                 threads=8, level=1):
    """write_results with results_z / results_r as the host copies of pack_results' output (uint8 [n, stride] streams,
    int64 lengths, CRCs): wc_write_test_results_packed stores them as they are."""
    n = len(out_paths)
    if n == 0:
        return
    zs, zl, zc, rs, rl, rc = packed
    for s, l, c in ((zs, zl, zc), (rs, rl, rc)):
        assert s.dtype == np.uint8 and s.ndim == 2 and s.flags['C_CONTIGUOUS'] and s.shape[0] >= n
        assert l.dtype == np.int64 and len(l) >= n and c.dtype.itemsize == 4 and len(c) >= n
    big = (_lib.ptr(zs), zs.shape[1], _lib.ptr(zl), _lib.ptr(zc), _lib.ptr(rs), rs.shape[1], _lib.ptr(rl), _lib.ptr(rc),
           int(member_bytes))
    _native_write(_lib.load().wc_write_test_results_packed, out_paths, per_file_args, runtime, binsize, threshold_z, big,
                  cwz, calls, n_calls, asdef, threads, level)


def write_results(out_paths, per_file_args, runtime, binsize, threshold_z, chrom_sizes, z, r, cwz, calls, n_calls,
                  asdef, threads=8, level=1, encoder='host'):
    """One `test` output file per row through the library's C++ thread pool (wc_write_test_results):
    the keys, dtypes and shapes of writeTestOutput's files.  z, r: float64
    [n, sum(chrom_sizes)]; cwz [n, n_sel]; calls [n, max_calls, 5]; n_calls int32 [n]; asdef [n].
    encoder='gpu': z and r are tensors on the GPU and are deflated there (pack_results); only the streams come to the
    host.  The files load identical; their results_z / results_r members are coded differently."""
    n = len(out_paths)
    if n == 0:
        return
    if check_encoder(encoder, level) == 'gpu':
        members = wt.ResultMembers(chrom_sizes, z.device)
        packed = tuple(_host_array(t) for t in pack_results(members, z, r))
        write_packed(out_paths, per_file_args, runtime, binsize, threshold_z, members.member_bytes, packed,
                     _host_array(cwz), _host_array(calls), _host_array(n_calls), _host_array(asdef), threads, level)
        return
    sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
    for a in (z, r):
        assert a.dtype == np.float64 and a.flags['C_CONTIGUOUS']
    assert z.shape[1] == int(sizes.sum())
    big = (_lib.ptr(sizes), len(sizes), _lib.ptr(z), _lib.ptr(r), z.shape[1])
    _native_write(_lib.load().wc_write_test_results, out_paths, per_file_args, runtime, binsize, threshold_z, big, cwz, calls,
                  n_calls, asdef, threads, level)


class _Staging(object):
    """Pinned host buffers of one in-flight batch."""

    def __init__(self, torch, batch, n_total, n_sel, max_calls, packed_stride=0):
        pin = dict(pin_memory=True)
        self.counts = torch.zeros((batch, n_total), dtype=torch.int32, **pin)
        if packed_stride:
            # the GPU encoder's route: the deflate streams of the two big members, their lengths and CRCs -- no z, no r
            self.streams = [torch.empty((batch * packed_stride,), dtype=torch.uint8, **pin) for _ in range(2)]
            self.lengths = [torch.empty((batch,), dtype=torch.int64, **pin) for _ in range(2)]
            self.crcs = [torch.empty((batch,), dtype=torch.int32, **pin) for _ in range(2)]
            self.packed = None
        else:
            self.z = torch.empty((batch, n_total), dtype=torch.float64, **pin)
            self.r = torch.empty((batch, n_total), dtype=torch.float64, **pin)
        self.cwz = torch.empty((batch, n_sel), dtype=torch.float64, **pin)
        self.calls = torch.empty((batch, max_calls, 5), dtype=torch.float64, **pin)
        self.n_calls = torch.empty((batch,), dtype=torch.int32, **pin)
        self.asdef = torch.empty((batch,), dtype=torch.float64, **pin)
        self.write_done = None     # future of the writer that still reads these buffers


def output_names(paths, outdir):
    """<outdir>/<leaf>_test.npz per input; two inputs with the same leaf name would overwrite each
    other's result, so that is an error up front."""
    names, seen = [], {}
    for path in paths:
        leaf = os.path.basename(path)
        leaf = leaf[:-4] if leaf.endswith('.npz') else leaf
        if leaf in seen:
            raise ValueError('testbatch: %s and %s would both be written to %s_test.npz; rename one of them'
                             % (seen[leaf], path, leaf))
        seen[leaf] = path
        names.append(os.path.join(outdir, leaf + '_test.npz'))
    return names


def run_testbatch(reference, paths, outdir, threshold, args, writer=None, max_calls=256, runtime=None):
    """`test` for every file of `paths` in GPU batches of args.batch samples.

    Pipeline per batch: decode (C++ thread pool) -> pinned counts -> H2D -> wc_test_batch_dev ->
    D2H into pinned results -> encode + write (C++ thread pool).  With args.encoder == 'gpu' the two big members
    (results_z, results_r) are assembled, deflated and CRC-summed on the device (pack_results) and only their streams
    come to the host; the thread pool then encodes the small members and writes.  The decode of batch i+1 and the
    writes of batch i-1 overlap the GPU work of batch i (two Python helper threads that only wait on
    the native calls, which release the GIL).  Returns timing figures (files, wall_s, files_per_s,
    gpu_s).  `writer(path, per_sample_args, result)`, when given, stores each result file in Python
    instead (the pre-native path, kept for comparison)."""
    import torch
    from .distributed import TestBatch
    began = time.time()
    n = len(paths)
    if n == 0:
        return dict(files=0, wall_s=0.0, files_per_s=0.0, gpu_s=0.0)
    dev = torch.device('cuda', reference.device)
    torch.cuda.set_device(dev)
    sizes = [int(v) for v in reference.chromosome_sizes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    sel = list(args.chromosomes)
    # wc_test_batch_dev takes at most 60000 (sample, chromosome) regions per call
    batch = max(1, min(int(args.batch), n, 60000 // max(1, len(sel))))
    io_threads = max(1, int(getattr(args, 'io', 8)))
    level = int(getattr(args, 'ziplevel', 1))
    on_gpu = check_encoder(getattr(args, 'encoder', 'host'), level) == 'gpu'
    if on_gpu and writer is not None:
        raise ValueError('the GPU encoder writes through the native writer: no `writer`')
    outs = output_names(paths, outdir)
    members = wt.ResultMembers(sizes, dev) if on_gpu else None
    packed_stride = wt.deflateBound(members.member_bytes) if on_gpu else 0
    stage = [_Staging(torch, batch, reference.n_total, len(sel), max_calls, packed_stride) for _ in range(2)]
    dev_counts = torch.zeros((batch, reference.n_total), dtype=torch.int32, device=dev)

    def new_batch(counts, calls_cap):
        return TestBatch(reference, counts, threshold, minrefbins=args.minrefbins, repeats=args.repeats,
                         chromosomes=sel, max_calls=calls_cap, mineffectsize=args.mineffectsize)
    tb = new_batch(dev_counts, max_calls)
    helpers = concurrent.futures.ThreadPoolExecutor(max_workers=2)
    py_writers = concurrent.futures.ThreadPoolExecutor(max_workers=io_threads) if writer else None
    gpu_s = wait_s = run_s = d2h_s = 0.0      # the GPU section and its parts: waiting for the result writers' buffers,
                                              # H2D + wc_test_batch_dev, D2H of the results
    pending = []

    def start_decode(at, slot):
        names = paths[at:at + batch]
        rows = stage[slot].counts.numpy()               # (the result writers never touch the counts buffer)
        return at, names, helpers.submit(read_counts, names, sizes, reference.binsize, rows, io_threads)

    def emit(at, names, slot, ns):
        st = stage[slot]
        per_file = []
        for i, name in enumerate(names):
            # what one `test` call would record: its own infile / outfile, not the batch's whole file list
            one = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in ('infiles', 'func')})
            one.infile = name
            one.outfile = outs[at + i]
            per_file.append(one)
        if on_gpu:
            st.write_done = helpers.submit(
                write_packed, outs[at:at + ns], per_file, runtime, reference.binsize, threshold, members.member_bytes,
                st.packed, st.cwz.numpy()[:ns], st.calls.numpy()[:ns], st.n_calls.numpy()[:ns], st.asdef.numpy()[:ns],
                io_threads, level)
            pending.append(st.write_done)
            return
        if writer is None:
            st.write_done = helpers.submit(
                write_results, outs[at:at + ns], per_file, runtime, reference.binsize, threshold, sizes,
                st.z.numpy()[:ns], st.r.numpy()[:ns], st.cwz.numpy()[:ns], st.calls.numpy()[:ns],
                st.n_calls.numpy()[:ns], st.asdef.numpy()[:ns], io_threads, level)
            pending.append(st.write_done)
            return
        z, r = st.z.numpy(), st.r.numpy()
        cwz, calls, n_calls, asdef = st.cwz.numpy(), st.calls.numpy(), st.n_calls.numpy(), st.asdef.numpy()
        for i, one in enumerate(per_file):
            result = dict(
                results_z=[z[i, offs[c]:offs[c + 1]].copy() for c in range(len(sizes))],
                results_r=[r[i, offs[c]:offs[c + 1]].copy() for c in range(len(sizes))],
                results_cwz=cwz[i].copy(), results_calls=calls[i, :n_calls[i]].copy(), asdef=float(asdef[i]))
            pending.append(py_writers.submit(writer, one.outfile, one, result))

    try:
        nxt = start_decode(0, 0)
        for bi, at in enumerate(range(0, n, batch)):
            slot = bi & 1
            at_, names, fut = nxt
            fut.result()
            if at + batch < n:
                nxt = start_decode(at + batch, slot ^ 1)
            ns = len(names)
            t0 = time.time()
            st = stage[slot]
            if st.write_done is not None:
                st.write_done.result()                  # the writer of two batches ago is done with these buffers
                st.write_done = None
            wait_s += time.time() - t0
            t1 = time.time()
            while True:
                dev_counts[:ns].copy_(st.counts[:ns], non_blocking=True)
                run = tb if ns == batch else new_batch(dev_counts[:ns], tb.max_calls)
                try:
                    run.run()
                except _lib.WisecondorHipError as exc:
                    # a sample with more calls than the output holds (e.g. hardly any reads):
                    # the reference has no such limit, so run the batch again with more room
                    if getattr(exc, 'code', 0) == _lib.E_LIMIT and 'max_calls' in str(exc) \
                            and tb.max_calls < reference.n_total:
                        grown = tb.max_calls * 4
                        tb = new_batch(dev_counts, grown)
                        for s_ in (0, 1):
                            if stage[s_].write_done is not None:
                                stage[s_].write_done.result()
                                stage[s_].write_done = None
                            stage[s_].calls = torch.empty((batch, grown, 5), dtype=torch.float64, pin_memory=True)
                        continue
                    raise
                break
            torch.cuda.synchronize()
            run_s += time.time() - t1
            t2 = time.time()
            if on_gpu:
                # encode on the device; the lengths first (how much of every stream there is to copy), then the streams
                # cut to the longest, the rows packed
                dev_packed = pack_results(members, run.results_z, run.results_r, ctx=reference.ctx)
                for m in (0, 1):
                    st.lengths[m][:ns].copy_(dev_packed[3 * m + 1], non_blocking=True)
                    st.crcs[m][:ns].copy_(dev_packed[3 * m + 2], non_blocking=True)
                torch.cuda.synchronize()
                st.packed = ()
                for m in (0, 1):
                    longest = max(1, int(st.lengths[m][:ns].max()))
                    host = st.streams[m][:ns * longest].view(ns, longest)
                    host.copy_(dev_packed[3 * m][:, :longest], non_blocking=True)
                    st.packed += (host.numpy(), st.lengths[m].numpy()[:ns], st.crcs[m].numpy()[:ns])
            else:
                st.z[:ns].copy_(run.results_z, non_blocking=True)
                st.r[:ns].copy_(run.results_r, non_blocking=True)
            st.cwz[:ns].copy_(run.cwz, non_blocking=True)
            st.calls[:ns].copy_(run.calls, non_blocking=True)
            st.n_calls[:ns].copy_(run.n_calls, non_blocking=True)
            st.asdef[:ns].copy_(run.asdef, non_blocking=True)
            torch.cuda.synchronize()
            d2h_s += time.time() - t2
            gpu_s += time.time() - t0
            emit(at, names, slot, ns)
        for f in pending:
            f.result()
    finally:
        helpers.shutdown(wait=True)
        if py_writers:
            py_writers.shutdown(wait=True)
    wall = time.time() - began
    return dict(files=n, wall_s=wall, files_per_s=n / wall if wall > 0 else 0.0, gpu_s=gpu_s,
                wait_writers_s=wait_s, h2d_and_kernels_s=run_s, d2h_s=d2h_s)


# ------------------------------------------------------------------------------------------ plotbatch ----
def plot_output_names(paths, outdir, filetype='png', command='plotbatch'):
    """<outdir>/<stem>_z.<filetype> per input (upstream's outfile + '_z.' + filetype); two inputs with the same stem are
    an error up front."""
    names, seen = [], {}
    for path in paths:
        stem = os.path.basename(path)
        stem = stem[:-4] if stem.endswith('.npz') else stem
        if stem in seen:
            raise ValueError('%s: %s and %s would both be written to %s_z.%s; rename one of them'
                             % (command, seen[stem], path, stem, filetype))
        seen[stem] = path
        names.append(os.path.join(outdir, '%s_z.%s' % (stem, filetype)))
    return names


def _load_result(path):
    """What `plotbatch` needs of a result file, or the exception that reading it raised."""
    try:
        with np.load(path, allow_pickle=True, encoding='latin1') as f:
            return dict(results_z=[np.asarray(c, dtype=np.float64) for c in f['results_z']],
                        results_calls=np.asarray(f['results_calls'], dtype=np.float64),
                        threshold_z=np.asarray(f['threshold_z']).item(), binsize=np.asarray(f['binsize']).item())
    except Exception as exc:           # reported by name, the run goes on
        return exc


def _write_bytes(path, data):
    """`data` to the file `path`; a tuple of names takes a tuple of files."""
    if isinstance(path, tuple):
        for one, part in zip(path, data):
            _write_bytes(one, part)
        return
    with open(path, 'wb') as f:
        f.write(data)


def _draw_png(results, names, table, args, device):
    return wt.plot_batch(results, names, cytofile=table, chromosomes=args.chromosomes, columns=args.columns, size=args.size,
                         mineffect=args.mineffect, dpi=getattr(args, 'dpi', 100), device=device)


def _draw_pdf(results, names, table, args, device):
    return wt.plot_pdf_batch(results, names, cytofile=table, chromosomes=args.chromosomes, columns=args.columns, size=args.size,
                             mineffect=args.mineffect, device=device)


def run_plotbatch(paths, outdir, args, device=0):
    """`plotbatch`: one PNG per result file, in GPU batches of args.batch samples (wt.plot_batch).  The files of batch
    i + 1 are read (np.load in the I/O thread pool) and the files of batch i - 1 written while batch i is on the GPU.
    Every file must share the chromosome lengths and the bin size of the first readable one; one that does not, or
    cannot be read, is named and skipped.  A -chromosomes entry the files do not hold is a ValueError.  Returns (files written, [(path, reason)] skipped, wall seconds)."""
    return _run_plots(paths, outdir, args, device, 'plotbatch', getattr(args, 'filetype', 'png'), _draw_png)


def run_plotpdf(paths, outdir, args, device=0):
    """`plotpdf`: one vector PDF per result file (wt.plot_pdf_batch), by run_plotbatch's pipeline and rules."""
    return _run_plots(paths, outdir, args, device, 'plotpdf', 'pdf', _draw_pdf)


def export_output_names(paths, outdir, gz=False):
    """<outdir>/<stem>.json (.json.gz) per input; two inputs with the same stem are an error up front."""
    names, seen = [], {}
    ending = 'json.gz' if gz else 'json'
    for path in paths:
        stem = os.path.basename(path)
        stem = stem[:-4] if stem.endswith('.npz') else stem
        if stem in seen:
            raise ValueError('exportjson: %s and %s would both be written to %s.%s; rename one of them' % (seen[stem], path, stem, ending))
        seen[stem] = path
        names.append(os.path.join(outdir, '%s.%s' % (stem, ending)))
    return names


def _load_export(path):
    """What `exportjson` writes of a result file, or the exception that reading it raised.  `arguments` whose pickle
    does not load here (a function of another program, stored by reference) are exported as {}."""
    try:
        with np.load(path, allow_pickle=True, encoding='latin1') as f:
            res = dict(results_z=[np.asarray(c, dtype=np.float64) for c in f['results_z']],
                       results_r=[np.asarray(c, dtype=np.float64) for c in f['results_r']],
                       results_calls=np.asarray(f['results_calls'], dtype=np.float64),
                       results_cwz=np.asarray(f['results_cwz'], dtype=np.float64))
            for key in ('binsize', 'threshold_z', 'asdef', 'aasdef'):
                res[key] = np.asarray(f[key]).item()
            try:
                arguments = f['arguments'].item()
            except Exception:
                arguments = {}
            res['arguments'] = arguments if isinstance(arguments, dict) else {}
            if [len(c) for c in res['results_r']] != [len(c) for c in res['results_z']]:
                raise ValueError('results_r and results_z differ in their chromosome lengths')
            return res
    except Exception as exc:           # reported by name, the run goes on
        return exc


def run_exportjson(paths, outdir, args, device=0):
    """`exportjson`: one JSON file per result file (wt.export_json_batch), by run_plotbatch's pipeline and rules."""
    def draw(results, names, table, args, device):
        return wt.export_json_batch(results, strict=bool(getattr(args, 'strict', False)), gz=bool(getattr(args, 'gz', False)), device=device)
    return _run_plots(paths, outdir, args, device, 'exportjson', 'json', draw, load=_load_export,
                      outs=export_output_names(paths, outdir, bool(getattr(args, 'gz', False))))


def tracks_output_names(paths, outdir, gz=False, only=None):
    """Per input the tuple (<outdir>/<stem>_z.bedgraph, <stem>_r.bedgraph, <stem>_calls.bed), the tracks .bedgraph.gz with
    gz and one of them alone with only = 'z' or 'r'; two inputs with the same stem are an error up front."""
    names, seen = [], {}
    ending = 'bedgraph.gz' if gz else 'bedgraph'
    for path in paths:
        stem = os.path.basename(path)
        stem = stem[:-4] if stem.endswith('.npz') else stem
        if stem in seen:
            raise ValueError('exporttracks: %s and %s would both be written to %s_calls.bed; rename one of them' % (seen[stem], path, stem))
        seen[stem] = path
        tracks = [os.path.join(outdir, '%s_%s.%s' % (stem, key, ending)) for key in wt.TRACKS if only in (None, key)]
        names.append(tuple(tracks) + (os.path.join(outdir, '%s_calls.bed' % stem),))
    return names


def read_chrom_sizes(path):
    """A chromosome sizes file (name<TAB>length per line, further columns ignored) as {name: length}; ValueError for a
    file that cannot be read or a line that is not that."""
    lengths = {}
    try:
        with open(path) as f:
            for number, line in enumerate(f, 1):
                if not line.strip() or line.startswith('#'):
                    continue
                fields = line.rstrip('\r\n').split('\t')
                if len(fields) < 2 or not fields[1].strip().isdigit():
                    raise ValueError('line %d is not name<TAB>length' % number)
                lengths[fields[0]] = int(fields[1])
    except (OSError, ValueError) as exc:
        raise ValueError('exporttracks: -chromsizes %s: %s' % (path, exc))
    return lengths


def chrom_lengths_for(lengths, prefix, sizes, binsize, path='the -chromsizes file'):
    """The lengths of the chromosomes <prefix>1 .. <prefix>n in the order of `sizes` (their bin counts); ValueError if one
    is missing or a chromosome's last bin starts at or beyond its length."""
    out = []
    for i, bins in enumerate(sizes):
        name = '%s%d' % (prefix, i + 1)
        if name not in lengths:
            raise ValueError('exporttracks: %s has no chromosome %s' % (path, name))
        if bins > 0 and (bins - 1) * binsize >= lengths[name]:
            raise ValueError('exporttracks: %s gives %s %d bases, the result files have %d bins of %d in it'
                             % (path, name, lengths[name], bins, binsize))
        out.append(lengths[name])
    return out


def _load_tracks(path):
    """What `exporttracks` writes of a result file, or the exception that reading it raised."""
    try:
        with np.load(path, allow_pickle=True, encoding='latin1') as f:
            res = dict(results_z=[np.asarray(c, dtype=np.float64) for c in f['results_z']],
                       results_r=[np.asarray(c, dtype=np.float64) for c in f['results_r']],
                       results_calls=np.asarray(f['results_calls'], dtype=np.float64))
            binsize = np.asarray(f['binsize']).item()
            if isinstance(binsize, bool) or not isinstance(binsize, (int, float)) or not binsize >= 1 or binsize != int(binsize):
                raise ValueError('its bin size %r is not a positive whole number' % (binsize,))
            res['binsize'] = int(binsize)
            if [len(c) for c in res['results_r']] != [len(c) for c in res['results_z']]:
                raise ValueError('results_r and results_z differ in their chromosome lengths')
            return res
    except Exception as exc:           # reported by name, the run goes on
        return exc


def run_exporttracks(paths, outdir, args, device=0, stats=None):
    """`exporttracks`: two bedGraph tracks and a BED file of the calls per result file (wt.export_tracks_batch), by
    run_plotbatch's pipeline and rules.  args.chromsizes: a chromosome sizes file whose lengths clip the ends; it is
    checked against the first readable file (ValueError).  stats: a dict whose 'dropped' grows by the bins left out as
    not finite."""
    gz, only = bool(getattr(args, 'gz', False)), getattr(args, 'only', None)
    prefix = getattr(args, 'chrprefix', 'chr')
    table = read_chrom_sizes(args.chromsizes) if getattr(args, 'chromsizes', None) else None
    clip = []

    def draw(results, names, cytobands, args, device):
        if table is not None and not clip:
            clip.append(chrom_lengths_for(table, prefix, [len(c) for c in results[0]['results_z']], results[0]['binsize'], args.chromsizes))
        details = {}
        files = wt.export_tracks_batch(results, only=only, gz=gz, nozero=bool(getattr(args, 'nozero', False)), prefix=prefix,
                                       chrom_lengths=clip[0] if clip else None, mineffect=getattr(args, 'mineffect', 0), device=device,
                                       details=details)
        if stats is not None:
            stats['dropped'] = stats.get('dropped', 0) + sum(sum(counts) for counts in details['dropped'])
        return files
    return _run_plots(paths, outdir, args, device, 'exporttracks', 'bedgraph', draw, load=_load_tracks,
                      outs=tracks_output_names(paths, outdir, gz, only))


def _run_plots(paths, outdir, args, device, command, filetype, draw, load=_load_result, outs=None):
    """The read / draw / write pipeline of `plotbatch`, `plotpdf`, `exportjson` and `exporttracks`: draw(results, names,
    cytoband table, args, device) returns the files' bytes; load(path) a result or the exception; outs the files' names
    (a tuple of names per input where draw returns a tuple of files per result)."""
    began = time.time()
    outs = plot_output_names(paths, outdir, filetype, command) if outs is None else outs
    batch = max(1, int(getattr(args, 'batch', 64)))
    io_threads = max(1, int(getattr(args, 'io', 8)))
    table = wt.loadCytoBands(args.cytofile) if getattr(args, 'cytofile', None) else None      # once, not once per panel
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=io_threads)
    skipped, writes, shape = [], [], None
    try:
        def start_read(at):
            return [pool.submit(load, p) for p in paths[at:at + batch]]
        ahead = start_read(0)
        for at in range(0, len(paths), batch):
            loaded = [f.result() for f in ahead]
            if at + batch < len(paths):
                ahead = start_read(at + batch)
            keep = []
            for k, res in enumerate(loaded):
                path = paths[at + k]
                if isinstance(res, Exception):
                    skipped.append((path, 'cannot be read: %s' % res))
                    continue
                mine = ([len(c) for c in res['results_z']], res['binsize'])
                if shape is None:
                    shape = mine
                    beyond = [c for c in getattr(args, 'chromosomes', ()) if not 1 <= c <= len(mine[0])]
                    if beyond:
                        raise ValueError('%s: -chromosomes names %s, %s holds chromosomes 1..%d'
                                         % (command, ','.join(str(c) for c in beyond), path, len(mine[0])))
                if mine[0] != shape[0]:
                    skipped.append((path, 'other chromosome lengths than the first file'))
                elif mine[1] != shape[1]:
                    skipped.append((path, 'bin size %s, the first file has %s' % (mine[1], shape[1])))
                else:
                    keep.append((at + k, res))
            if not keep:
                continue
            files = draw([res for _, res in keep], [wt.sampleNameOf(paths[i]) for i, _ in keep], table, args, device)
            writes.extend(pool.submit(_write_bytes, outs[i], data) for (i, _), data in zip(keep, files))
        for job in writes:
            job.result()
    finally:
        pool.shutdown(wait=True)
    return len(writes), skipped, time.time() - began
