"""Command line of the MI355X build: the `convert`, `newref*`, `test` and `report` sub-commands of WISECONDOR.

Contract (taken from the upstream CLI at
wisecondor.py:345-521): same sub-command names, positional arguments, single-dash
options, defaults and `dest` names; same file naming (`<stem>_prep.npz`,
`<stem>_part_<m>.npz`, resume by file existence, temporaries removed after a
successful merge); same `.npz` keys and dtypes; `test` ends with exit status 0.
Everything numeric runs on the GPU through libwisecondor_hip.so (no CPU path).

Build-only additions, all off by default: `-gpus N` on `newref` / `testbatch`
(one process per GPU), the `testbatch` sub-command (many samples per GPU batch), the `convertbatch`
sub-command (many BAM files, reading file i + 1 while file i is on the GPU and file i - 1 is written), the
`plotbatch` sub-command (result files to z-score panel PNGs, drawn and deflated on the GPU), the `plotpdf`
sub-command (the same panels as vector PDF pages, the content stream written on the GPU), the `exportjson`
sub-command (result files to lossless JSON, the numbers' digits made on the GPU) and the `exporttracks` sub-command
(result files to bedGraph tracks and BED calls for genome browsers, the text and its BGZF blocks made on the GPU) and
the `sensitivity` sub-command (aberrations planted into healthy samples on the GPU, tested and judged there: how often
a reference finds a span of a given length and effect, at the samples' read depth or thinned to fractions of it) and
the `downsample` sub-command (a converted sample thinned to a fraction of its reads on the GPU) and the `crossval`
sub-command (every healthy sample tested against a reference built without its fold, the held-out z-scores judged on
the GPU).
`plot` itself stays refused: its default output is a matplotlib PDF, which this build does not make.
"""
import argparse
import copy
import datetime
import getpass
import os
import socket
import subprocess
import sys
import time

import numpy as np
from scipy.stats import norm

from . import wisetools as wt

_STARTED = datetime.datetime.now()


# ------------------------------------------------------------------ provenance ----
_VERSION_TAG = []


def getRuntime():
    """The `runtime` member of every output file: version, datetime, hostname, username
    (upstream wisetools.py:47-62).  `git describe` runs once per process."""
    if not _VERSION_TAG:
        try:
            _VERSION_TAG.append(subprocess.check_output(["git", "describe", "--always"], stderr=subprocess.DEVNULL).split()[0])
        except Exception:
            _VERSION_TAG.append('unknown')
    tag = _VERSION_TAG[0]
    return {'version': tag, 'datetime': _STARTED, 'hostname': socket.gethostname(),
            'username': getpass.getuser()}


def printArgs(args):
    """Echo the parsed command (tool name first, then the options in name order)."""
    settings = dict(vars(args))
    tool = settings.pop('func', None)
    print('tool =', getattr(tool, '__name__', str(tool)).replace('tool', '', 1))
    for name in sorted(settings):
        print(name, '=', settings[name])


def _open_npz(path):
    return np.load(path, allow_pickle=True, encoding='latin1')


def _as_object_array(arrays):
    """Ragged per-chromosome arrays as one object array (numpy >= 1.24 no longer infers it)."""
    boxed = np.empty(len(arrays), dtype=object)
    for at, item in enumerate(arrays):
        boxed[at] = item
    return boxed


# --------------------------------------------------------------------- convert ----
def writeConvertOutput(outfile, args, converted, qual_info):
    """The `convert` output file (wisecondor.py:22-26; keys of SURVEY.md App. B)."""
    write_npz(outfile, arguments=vars(args), runtime=getRuntime(), sample=converted, quality=qual_info)


def _convert_route(args):
    """The route `convert` / `convertbatch` take: 'bounded' (-bounded: chunk by chunk through the reader AND the filters),
    'stream' (-stream: the streamed reader, the filters on the whole arrays) or 'whole'.  `-chunk` is the option of the
    two chunked routes: without one of them it is an error, not something to ignore and then record in the output
    file's `arguments`."""
    bounded, streamed = getattr(args, 'bounded', False), getattr(args, 'stream', False)
    if bounded and streamed:
        raise ValueError('-stream and -bounded are two routes: give one of them')
    route = 'bounded' if bounded else 'stream' if streamed else \
        wt.CONVERT_READER if wt.CONVERT_READER in ('stream', 'bounded') else 'whole'
    if hasattr(args, 'chunk') and route == 'whole':
        raise ValueError('-chunk sets the chunk size of the streamed reader: give -stream (or -bounded) as well')
    return route


def _convert_streamed(args):
    """True where `convert` / `convertbatch` read through the streamed reader (_convert_route: 'stream')."""
    return _convert_route(args) == 'stream'


def _convert_bounded(args, path, verbose):
    return wt.convertBamBounded(path, args.binsize, args.retdist, args.retthres, mapq=getattr(args, 'mapq', 1),
                                demandPair=getattr(args, 'paired', False), chunk=getattr(args, 'chunk', 0), verbose=verbose)


def toolConvert(args):
    """`convert infile outfile`: BAM -> binned, filtered sample (wisecondor.py:20-27)."""
    route = _convert_route(args)
    if route == 'bounded':
        # build-only: reader and filters chunk by chunk, no per-read arrays (memory does not grow with the read count)
        converted, qual_info = _convert_bounded(args, args.infile, True)
    elif route == 'stream':
        # build-only: the streamed device reader (memory bounded by the chunk); the same filters and binning behind it
        with wt.openBamReads(args.infile, stream=True, chunk=getattr(args, 'chunk', 0)) as bam:
            converted, qual_info = wt.convertBamReads(bam, args.binsize, args.retdist, args.retthres, verbose=True,
                                                      mapq=getattr(args, 'mapq', 1),
                                                      demandPair=getattr(args, 'paired', False))
    else:
        converted, qual_info = wt.convertBam(args.infile, binsize=args.binsize, minShift=args.retdist,
                                             threshold=args.retthres, mapq=getattr(args, 'mapq', 1),
                                             demandPair=getattr(args, 'paired', False))
    writeConvertOutput(args.outfile, args, converted, qual_info)
    print('Conversion finished')


def convert_output_names(paths, outdir):
    """<outdir>/<leaf without .bam>.npz per input; two inputs with the same leaf name are an error up front."""
    names, seen = [], {}
    for path in paths:
        leaf = os.path.basename(path)
        leaf = leaf[:-4] if leaf.lower().endswith('.bam') else leaf
        if leaf in seen:
            raise ValueError('convertbatch: %s and %s would both be written to %s.npz; rename one of them'
                             % (seen[leaf], path, leaf))
        seen[leaf] = path
        names.append(os.path.join(outdir, leaf + '.npz'))
    return names


def toolConvertBatch(args):
    """`convertbatch infiles... outdir` (build-only): the same file per BAM as one `convert` each.  A reader thread
    runs the host stage (file into pinned memory, block directory, header: native code, no GIL) of file i + 1 and a
    writer thread stores file i - 1 while file i is on the GPU; the device stage of the reader runs on this thread."""
    import argparse
    import concurrent.futures
    outs = convert_output_names(args.infiles, args.outdir)
    os.makedirs(args.outdir, exist_ok=True)
    began = time.time()
    reader = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    writer = concurrent.futures.ThreadPoolExecutor(max_workers=1)
    written = []
    ahead = taken = None
    try:
        # the reader thread's share: the host stage of the device reader, or the whole host reader; nothing for the
        # streamed reader, which has a reader thread of its own and holds no file whole
        route = _convert_route(args)
        streamed = route == 'stream'
        if route != 'whole':
            stage = None
        elif wt.CONVERT_READER == 'device':
            def stage(path):
                return wt.BamFile(path)
        else:
            def stage(path):
                return wt.BamReads(path, args.io)
        if stage:
            ahead = reader.submit(stage, args.infiles[0])
        for i, (path, out) in enumerate(zip(args.infiles, outs)):
            if route == 'bounded':
                bam = None
            elif streamed:
                bam = wt.openBamReads(path, stream=True, chunk=getattr(args, 'chunk', 0))
            else:
                bam = ahead.result()
                taken = ahead
                if i + 1 < len(args.infiles):
                    ahead = reader.submit(stage, args.infiles[i + 1])
            if isinstance(bam, wt.BamFile):
                bamfile = bam
                try:
                    bam = wt.openBamReads(bamfile, threads=args.io)     # the device stage, on this thread
                finally:
                    bamfile.close()
            try:
                if bam is None:
                    converted, qual_info = _convert_bounded(args, path, False)
                else:
                    converted, qual_info = wt.convertBamReads(bam, args.binsize, args.retdist, args.retthres,
                                                              mapq=getattr(args, 'mapq', 1),
                                                              demandPair=getattr(args, 'paired', False))
            finally:
                if bam is not None:
                    bam.close()
            # what one `convert` call would record: its own infile / outfile, not the batch's list
            one = argparse.Namespace(**{k: v for k, v in vars(args).items() if k not in ('infiles', 'outdir', 'io', 'func')})
            one.infile, one.outfile, one.func = path, out, toolConvert
            written.append(writer.submit(writeConvertOutput, out, one, converted, qual_info))
        for job in written:
            job.result()
    finally:
        reader.shutdown(wait=True)
        writer.shutdown(wait=True)
        # a file the read-ahead thread opened and the loop never took (it left on an exception): release its buffers
        if ahead is not None and ahead is not taken and ahead.exception() is None:
            ahead.result().close()
    print('%d BAM files converted in %.2f s' % (len(outs), time.time() - began))


# ---------------------------------------------------------------------- report ----
def toolReport(args):
    """`report testfile resultfile`: the text summary of a `convert` file and a `test` file, line for line what
    wisecondor.py:304-342 prints."""
    test_file = _open_npz(args.testfile)
    result_file = _open_npz(args.resultfile)
    binSize = result_file['binsize'].item()

    print('\n# Arguments used in convert: #')
    test_args = test_file['arguments'].item()
    for key in test_args:
        print(key, '=', test_args[key])
    print('\n# Arguments used in test: #')
    result_args = result_file['arguments'].item()
    for key in result_args:
        print(key, '=', result_args[key])

    quality = test_file['quality'].item()
    print('\n# BAM information: #')
    print('Reads mapped:  \t', quality['mapped'])
    print('Reads unmapped:\t', quality['unmapped'])
    print('Reads nocoord: \t', quality['no_coordinate'])
    print('Reads rmdup:   \t', quality['filter_rmdup'])
    print('Reads lowqual: \t', quality['filter_mapq'])

    reads_in = quality['pre_retro'] - quality['no_coordinate'] + quality['filter_rmdup'] + quality['filter_mapq']
    print('\n# RETRO filtering: #')
    print('Reads in:     \t', reads_in)
    print('Reads removed:\t', reads_in - quality['post_retro'])
    print('Reads out:    \t', quality['post_retro'])

    print('\n# Z-Score checks: #')
    print('Z-Score used:\t', "{:.2f}".format(result_file['threshold_z'].item()))
    print('AvgStdDev:   \t', "{:.2f}".format(result_file['asdef'] * 100) + '%')
    print('AvgAllStdDev:\t', "{:.2f}".format(result_file['aasdef'] * 100) + '%')

    print('\n# Test results: #')
    print('z-score\teffect\tmbsize\tlocation')
    for result in result_file['results_calls']:
        if args.mineffect < abs(result[4] * 100):
            print("{:.2f}\t{:.2f}\t{:.2f}\t{:.0f}:{:.0f}-{:.0f}".format(
                result[3], result[4] * 100, (result[2] - result[1] + 1) * binSize / 1e6, result[0],
                result[1] * binSize, (result[2] + 1) * binSize))


# --------------------------------------------------------------- newref: files ----
class BuildFiles(object):
    """Names of the intermediate files of one `newref` job.

    `reference.npz` -> `reference_prep.npz` and `reference_part_<m>.npz` (a trailing `.npz`
    of the output name is dropped first; upstream wisecondor.py:31-39).
    """

    def __init__(self, outfile):
        folder, leaf = os.path.split(outfile)
        if leaf.endswith('.npz'):
            leaf = leaf[:-len('.npz')]
        stem = os.path.join(folder, leaf)
        self.prep = stem + '_prep.npz'
        self.part_base = stem + '_part'

    @staticmethod
    def part_name(part_base, number):
        return '%s_%d.npz' % (part_base, number)


def _missing_parts(part_base, parts):
    return [m for m in range(1, parts + 1) if not os.path.isfile(BuildFiles.part_name(part_base, m))]


def _visible_gpus():
    import torch
    return int(torch.cuda.device_count())      # counting devices does not initialise the runtime


def _rank_count(args):
    """Processes (= GPUs) a `newref` / `testbatch` run uses.

    `-gpus N` asks for N; without it `-cpus N` (the upstream worker-pool size) is honoured up to
    the number of visible GPUs.  One rank runs in this process, more are started as children
    (wisecondor_amd.ranks) before anything here touches the GPU."""
    want = getattr(args, 'gpus', None)
    if want is None:
        want = min(max(1, int(getattr(args, 'cpus', 1))), max(1, _visible_gpus()))
    if want < 1:
        print('ERROR: -gpus needs a positive count, got', want)
        sys.exit(1)
    return int(want)


def write_npz(path, temporary=False, **arrays):
    """The .npz files of this tool (np.load reads them like np.savez_compressed's, which the
    reference uses: wisecondor.py:97-108, 128-132, 160-170).  Once the GPU part takes
    milliseconds the sub-commands' wall time is zlib (1.7 of 1.8 s of `newref` at 100 x 250 kb),
    so members are deflated at level 1 in threads (wisecondor_amd/npzfast.py; WC_NPZ_LEVEL=6 for
    numpy's own level) and the prep / part files `newref` deletes again at its end are stored."""
    from . import npzfast
    level = 0 if temporary else int(os.environ.get('WC_NPZ_LEVEL', '1'))
    npzfast.savez(path, level=level, threads=min(16, os.cpu_count() or 1), **arrays)


def save_part(part_base, number, parts, indexes, distances, args, temporary=False):
    """One part file exactly as `newrefpart` writes it (keys of SURVEY.md App. B)."""
    stamped = copy.copy(args)
    stamped.part = [number, parts]
    write_npz(BuildFiles.part_name(part_base, number), temporary,
              arguments=vars(stamped),
              runtime=getRuntime(),
              indexes=indexes,
              distances=distances)


def part_owners(parts, numbers, n_bins, world):
    """Which rank owns each of the part files `numbers` (1-based) of `parts`: the rank whose row range
    (distributed.row_range = the reference's getPart for `world` parts) holds the part's rows; None when
    some part straddles two ranks' ranges (then every rank needs all rows)."""
    from .distributed import row_range
    ranges = [row_range(r, world, n_bins) for r in range(world)]
    owners = {}
    for m in numbers:
        lo, hi = wt.getPart(m - 1, parts, n_bins)
        own = [r for r, (b, e) in enumerate(ranges) if b <= lo and hi <= e]
        if hi <= lo:
            own = [r for r, (b, e) in enumerate(ranges) if b <= lo <= e] or [0]
        if not own:
            return None
        owners[m] = own[0]
    return owners


def select_all_rows(prepfile, refsize, device=0, rank=0, world=1, gather=True):
    """indexes / distances of every bin from a prep file, matrix resident on `device`.

    One NewrefJob pass (wisecondor_amd.distributed); with world > 1 the ranks share the work
    and each ends with the full result -- or, gather=False, with the rows it owns only (no result
    all-gather: the reference's workers exchange nothing but files, wisecondor.py:47-56)."""
    import torch
    from . import _lib
    from .distributed import NewrefJob
    prep = prepfile if isinstance(prepfile, dict) else _open_npz(prepfile)
    corrected = np.asarray(prep['correctedData'])
    bins = np.ascontiguousarray(prep['maskedChromBins'], dtype=np.int64)
    order = wt.sum_order_of(corrected)
    dev = torch.device('cuda', device)
    torch.cuda.set_device(dev)
    X = torch.from_numpy(np.ascontiguousarray(corrected, dtype=np.float64)).to(dev)
    job = NewrefJob(_lib.context(device), X, bins, int(refsize), order, rank=rank, world=world, gather=gather)
    idx, dst = job.run()
    torch.cuda.synchronize()
    return idx.cpu().numpy(), dst.cpu().numpy(), job


# --------------------------------------------------------------- newref: tools ----
def readBlacklistOption(args, chrom_sizes, binsize):
    """The bins `-blacklist FILE` drops at the layout chrom_sizes of `binsize` bp bins (blacklist.readBlacklist), or None
    without the option.  Prints how many bins are dropped and how many lines were ignored."""
    if getattr(args, 'blacklist', None) is None:
        return None
    from . import blacklist
    drop, ignored = blacklist.readBlacklist(args.blacklist, chrom_sizes, binsize)
    print('Blacklist %s: %d of %d bins dropped, %d lines ignored (not chromosome 1 .. 22)'
          % (args.blacklist, int(drop.sum()), len(drop), ignored))
    return drop


def toolNewrefPrep(args, temporary=False):
    """`newrefprep`: sample files -> prep file (normalise, mask all-zero bins, PCA-correct).

    File contract of upstream wisecondor.py:72-108; the arithmetic is wt.prepReference (GPU).
    Returns what it wrote (for `newref`, which goes on with the arrays instead of reading the
    file back)."""
    from . import ingest
    counts, chrom_bins_in, binsizes = ingest.load_counts(args.infiles, args.binsize, threads=min(16, os.cpu_count() or 1),
                                                         verbose=True)
    if args.binsize is None and len(binsizes) > 1:
        print('ERROR: the input samples were binned at different sizes:', sorted(binsizes))
        print('Drop the odd ones or give -binsize to merge them to a common size')
        sys.exit(1)
    binsize = args.binsize if args.binsize is not None else next(iter(binsizes))

    n_given = counts.shape[0]
    try:
        drop = readBlacklistOption(args, chrom_bins_in, binsize)
    except (ValueError, OSError) as exc:
        print('ERROR:', exc)
        sys.exit(1)
    masked, chrom_bins, mask, corrected, components, mean, masked_bins = wt.prepReference(
        None, counts=counts, chrom_bins=chrom_bins_in, drop=drop)
    print('Zero mask on the GPU: %d bins x %d samples -> %d bins kept, 3 PCA components removed'
          % (len(mask), n_given, masked.shape[0]))
    running = np.cumsum(masked_bins)
    stored = dict(arguments=vars(args),
                  runtime=getRuntime(),
                  binsize=binsize,
                  chromosomeBins=chrom_bins,
                  maskedData=masked,
                  mask=mask,
                  maskedChromBins=masked_bins,
                  maskedChromBinSums=[int(v) for v in running],
                  correctedData=corrected,
                  pca_components=components,
                  pca_mean=mean)
    if drop is not None:
        stored['blacklist'] = drop
    write_npz(args.prepfile, temporary, **stored)
    return stored


def toolNewrefPart(args):
    """`newrefpart prep part m n`: reference bins for row part m of n (1-based) -> `<part>_m.npz`."""
    number, parts = args.part
    if number > parts:
        print('ERROR: part number %d exceeds the part count %d' % (number, parts))
        sys.exit(1)
    if number < 0:
        print('ERROR: part number %d is negative' % number)
        sys.exit(1)
    prep = _open_npz(args.prepfile)
    began = time.time()
    indexes, distances = wt.getReference(prep['correctedData'], prep['maskedChromBins'],
                                         prep['maskedChromBinSums'], selectRefAmount=args.refsize,
                                         part=number, splitParts=parts)
    print('part %d of %d: %d rows in %.2f s' % (number, parts, indexes.shape[0], time.time() - began))
    save_part(args.partfile, number, parts, indexes, distances, args)


def toolNewrefPost(args):
    """`newrefpost prep part n out`: stack the n part files in order, add the prep file's layout."""
    prep = _open_npz(args.prepfile)
    idx_blocks, dst_blocks = [], []
    for number in range(1, args.parts + 1):
        name = BuildFiles.part_name(args.partfile, number)
        piece = _open_npz(name)
        idx_blocks.append(np.asarray(piece['indexes']))
        dst_blocks.append(np.asarray(piece['distances']))
        print('merged', name, idx_blocks[-1].shape)
    width = max(b.shape[1] for b in idx_blocks if b.ndim == 2) if any(b.ndim == 2 for b in idx_blocks) else 0
    idx_blocks = [b.reshape(-1, width) for b in idx_blocks]
    dst_blocks = [b.reshape(-1, width) for b in dst_blocks]
    # (a prep file made with -blacklist carries the dropped bins; the reference file then does too)
    extra = dict(blacklist=prep['blacklist']) if 'blacklist' in prep.files else {}
    write_npz(args.outfile,
              arguments=vars(args),
              runtime=getRuntime(),
              binsize=prep['binsize'].item(),
              indexes=np.concatenate(idx_blocks, axis=0),
              distances=np.concatenate(dst_blocks, axis=0),
              chromosome_sizes=prep['chromosomeBins'],
              mask=prep['mask'],
              masked_sizes=prep['maskedChromBins'],
              pca_components=prep['pca_components'],
              pca_mean=prep['pca_mean'],
              **extra)


def toolNewref(args):
    """`newref`: prep, every missing part, merge, clean up (upstream wisecondor.py:30-69).

    The upstream tool fans the parts over `-cpus` worker processes; here the rows are computed
    in one pass by one process per GPU (`-gpus`, default min(-cpus, visible GPUs)) and cut into
    the same part files, so an interrupted run resumes from whatever files exist."""
    names = BuildFiles(args.outfile)
    args.prepfile, args.partfile = names.prep, names.part_base
    args.parts = max(args.parts, args.cpus)
    ranks = _rank_count(args)
    todo = _missing_parts(args.partfile, args.parts)
    if ranks > 1 and (todo or not os.path.isfile(args.prepfile)):
        from . import ranks as rk
        rk.launch(ranks, dict(job='newref', prepfile=args.prepfile, partfile=args.partfile,
                              parts=args.parts, refsize=args.refsize, infiles=list(args.infiles),
                              binsize=args.binsize, arguments=_plain_arguments(args)))
    else:
        prep = None
        if not os.path.isfile(args.prepfile):
            prep = toolNewrefPrep(args, temporary=True)        # (the file is for a resumed run; this one keeps the arrays)
        if todo:
            began = time.time()
            indexes, distances, _ = select_all_rows(prep if prep is not None else args.prepfile, args.refsize)
            print('reference bins for %d rows in %.2f s' % (indexes.shape[0], time.time() - began))
            for number in todo:
                lo, hi = wt.getPart(number - 1, args.parts, indexes.shape[0])
                save_part(args.partfile, number, args.parts, indexes[lo:hi], distances[lo:hi], args, temporary=True)
    toolNewrefPost(args)
    os.remove(args.prepfile)
    for number in range(1, args.parts + 1):
        os.remove(BuildFiles.part_name(args.partfile, number))


def _plain_arguments(args):
    """vars(args) without the function object (for hand-over to worker processes as JSON)."""
    return {k: v for k, v in vars(args).items() if k != 'func'}


# ------------------------------------------------------------------------ test ----
def zThreshold(masked_sizes, multitest, minzscore):
    """Per-bin |z| cut of the first testing cycles: `-minzscore` if given, else the normal
    quantile for one expected false positive in bins/2 * multitest tests (wisecondor.py:203-207)."""
    if minzscore is not None:
        return minzscore
    tests = sum(masked_sizes) * 0.5 * multitest
    return norm.ppf(1 - 1. / tests)


def writeTestOutput(outfile, args, binsize, result, z_threshold):
    """The `test` output file (keys and shapes of SURVEY.md App. B): per-chromosome z and
    ratio-1 arrays as object arrays, calls [n, 5] (shape (0,) when empty), the thresholds."""
    calls = np.asarray(result['results_calls'])
    if calls.size == 0:
        calls = np.array([])
    write_npz(outfile,
              arguments=vars(args),
              runtime=getRuntime(),
              binsize=binsize,
              results_r=_as_object_array(result['results_r']),
              results_z=_as_object_array(result['results_z']),
              results_cwz=result['results_cwz'],
              results_calls=calls,
              threshold_z=z_threshold,
              asdef=result['asdef'],
              aasdef=result['asdef'] * z_threshold)


def _reference_and_threshold(args, device=0):
    stored = _open_npz(args.reference)
    reference = wt.Reference.from_npz(stored, device=device)
    cut = zThreshold([int(v) for v in stored['masked_sizes']], args.multitest, args.minzscore)
    print('z-score threshold per bin:', cut)
    return reference, cut


def toolTest(args):
    """`test sample out reference`: one sample against a reference (wisecondor.py:174-281)."""
    reference, cut = _reference_and_threshold(args)
    from . import ingest
    sample = ingest.read_sample(args.infile, reference.binsize)[0]
    began = time.time()
    result = wt.test_batch(reference, [sample], cut, minrefbins=args.minrefbins, repeats=args.repeats,
                           chromosomes=list(args.chromosomes), mineffectsize=args.mineffectsize)[0]
    print('ASDES:', result['asdef'])
    print('AASDEF:', result['asdef'] * cut)
    print('z-scores and segments took %.3f s' % (time.time() - began))
    writeTestOutput(args.outfile, args, reference.binsize, result, cut)
    reference.close()
    sys.exit(0)


def toolTestBatch(args):
    """`testbatch samples... outdir reference` (build-only): the same numbers and the same
    per-sample files as one `test` per sample, in GPU batches with pooled file decode / encode.
    `-gpus N` (or a torchrun environment) shards the sample list over N processes.  `-encoder gpu` deflates the two
    large members of every result file on the GPU (ingest.pack_results); it is refused with any -ziplevel but 1."""
    from . import ingest
    ingest.check_encoder(getattr(args, 'encoder', 'host'), getattr(args, 'ziplevel', 1))
    world_env = int(os.environ.get('WORLD_SIZE', '1'))
    if world_env == 1 and _rank_count(args) > 1:
        from . import ranks as rk
        rk.launch(_rank_count(args), dict(job='testbatch', arguments=_plain_arguments(args)))
        return
    from . import ingest
    from .distributed import shard_samples
    rank = int(os.environ.get('RANK', '0'))
    device = int(os.environ.get('LOCAL_RANK', '0')) % max(1, _visible_gpus())   # functional runs may share a GPU
    reference, cut = _reference_and_threshold(args, device=device)
    lo, hi = shard_samples(len(args.infiles), rank, world_env)
    os.makedirs(args.outdir, exist_ok=True)
    stats = ingest.run_testbatch(reference, args.infiles[lo:hi], args.outdir, cut, args, runtime=getRuntime())
    print('rank %d: %d samples in %.2f s (%.1f files/s end to end; GPU batches %.3f s = %.3f waiting for the result '
          'writers + %.3f copy in and kernels + %.3f results out)'
          % (rank, stats['files'], stats['wall_s'], stats['files_per_s'], stats['gpu_s'],
             stats.get('wait_writers_s', 0.0), stats.get('h2d_and_kernels_s', 0.0), stats.get('d2h_s', 0.0)))
    reference.close()


# ------------------------------------------------------------------- plotbatch, plotpdf, exportjson ----
def _run_result_tool(args, name_outputs, run, noun):
    """What the result-file tools do once their options are checked: name_outputs() refuses two inputs with one stem
    before anything is made, run(infiles, outdir, args) gives (written, skipped, seconds); the summary line counts `noun`
    (a text, or a function that gives it once the run is over), every skipped file is named, and one of them makes the
    exit status 1."""
    try:
        name_outputs()
        os.makedirs(args.outdir, exist_ok=True)
        written, skipped, wall = run(args.infiles, args.outdir, args)
    except ValueError as exc:
        print('ERROR:', exc)
        sys.exit(2)
    print('%d %s written in %.2f s (%.1f files/s end to end)' % (written, noun() if callable(noun) else noun, wall,
                                                                 written / wall if wall > 0 else 0.0))
    for path, reason in skipped:
        print('ERROR: %s skipped: %s' % (path, reason))
    if skipped:
        sys.exit(1)


def toolPlotBatch(args):
    """`plotbatch infiles... outdir` (build-only): <outdir>/<stem>_z.png per result file, what upstream `plot` draws
    (wisecondor.py:284-295) by this build's own rasteriser on the GPU.  A file that cannot be read, or whose chromosome
    lengths or bin size differ from the first file's, is named and skipped; the exit status is then 1."""
    if args.filetype != 'png':
        print('ERROR: plotbatch writes png only (-filetype %s asked for); upstream plot makes the other formats' % args.filetype)
        sys.exit(2)
    if args.columns < 1 or args.dpi < 1 or not args.chromosomes:
        print('ERROR: plotbatch needs -columns >= 1, -dpi >= 1 and at least one chromosome')
        sys.exit(2)
    from . import ingest
    _run_result_tool(args, lambda: ingest.plot_output_names(args.infiles, args.outdir, args.filetype), ingest.run_plotbatch, 'plots')


def toolPlotPdf(args):
    """`plotpdf infiles... outdir` (build-only): <outdir>/<stem>_z.pdf per result file, the name and the vector format of
    upstream `plot`'s default output (wisecondor.py:284-295), the page's content stream written on the GPU.  Files are
    treated as `plotbatch` treats them: one that cannot be read, or whose chromosome lengths or bin size differ from the
    first file's, is named and skipped; the exit status is then 1."""
    if args.columns < 1 or not args.chromosomes or min(args.size) <= 0:
        print('ERROR: plotpdf needs -columns >= 1, a -size above 0 and at least one chromosome')
        sys.exit(2)
    from . import ingest
    _run_result_tool(args, lambda: ingest.plot_output_names(args.infiles, args.outdir, 'pdf', 'plotpdf'), ingest.run_plotpdf, 'plots')


def toolExportJson(args):
    """`exportjson infiles... outdir` (build-only): <outdir>/<stem>.json (.json.gz with -gz) per result file, every
    number as json.dumps writes it, so that json.loads gives the stored doubles back bit for bit; the digits of
    results_z and results_r are made on the GPU.  Files are treated as `plotbatch` treats them: one that cannot be read,
    or whose chromosome lengths or bin size differ from the first file's, is named and skipped; the exit status is then 1."""
    from . import ingest
    _run_result_tool(args, lambda: ingest.export_output_names(args.infiles, args.outdir, args.gz), ingest.run_exportjson, 'files')


def toolExportTracks(args):
    """`exporttracks infiles... outdir` (build-only): <outdir>/<stem>_z.bedgraph, <stem>_r.bedgraph (.bedgraph.gz, BGZF,
    with -gz) and <stem>_calls.bed per result file, for genome browsers: a line per run of equal bins, every value as
    repr writes it; the tracks' text and the BGZF blocks are made on the GPU.  Files are treated as `exportjson` treats
    them; one whose bin size is no positive whole number is skipped too."""
    from . import ingest
    stats = {'dropped': 0}

    def name_outputs():
        wt._track_prefix(args.chrprefix)
        if args.chromsizes:
            ingest.read_chrom_sizes(args.chromsizes)
        return ingest.tracks_output_names(args.infiles, args.outdir, args.gz, args.only)
    _run_result_tool(args, name_outputs, lambda infiles, outdir, args: ingest.run_exporttracks(infiles, outdir, args, stats=stats),
                     lambda: 'result files as tracks (%d bins left out as not finite)' % stats['dropped'])


# ----------------------------------------------------------------- sensitivity ----
def sensitivityOutputs(outfile):
    """(out.npz, out.tsv) of the `out` argument (a trailing .npz is taken as part of neither)."""
    stem = outfile[:-4] if outfile.endswith('.npz') else outfile
    return stem + '.npz', stem + '.tsv'


def toolSensitivity(args):
    """`sensitivity healthy... out reference -lengths bp,... -effects percent,...` (build-only): spans of every length
    are planted at -trials random places into every healthy sample with every effect, each spiked copy is tested as
    `test` tests a sample, and every trial's calls are judged against what was planted, all on the GPU
    (wt.sensitivity_batch).  Writes out.npz (the plan, a record per trial, the table) and out.tsv (the table), and prints
    the table.  -depths thins the samples on the GPU to every fraction of their reads and repeats the grid per depth
    (the table gains a leading depth_ppm column and a control line per depth); -draw plants Binomial spikes instead of
    the rounded product; -seed keys both.  Everything that can be refused is refused before the GPU is touched: exit
    status 2."""
    from . import ingest, sensitivity
    try:
        stored = _open_npz(args.reference)
        binsize = stored['binsize'].item() if hasattr(stored['binsize'], 'item') else stored['binsize']
        lengths_bins, effects_ppm = sensitivity.parseGrid(args.lengths, args.effects, binsize)
        if args.trials < 1 or args.batch < 1 or not args.chromosomes or not 0 <= args.minoverlap <= 1:
            raise ValueError('sensitivity needs -trials >= 1, -batch >= 1, -minoverlap in 0 .. 1 and at least one chromosome')
        for path in args.infiles:
            own = _open_npz(path)['arguments'].item()['binsize']
            if own == 0 or binsize < own or binsize % own > 0:
                raise ValueError('%s was binned at %s, which does not scale to the reference\'s %s' % (path, own, binsize))
        depths_ppm = sensitivity.parseDepths(args.depths) if hasattr(args, 'depths') else None
        draw = bool(getattr(args, 'draw', False))
        plan = sensitivity.makePlan(stored, len(args.infiles), lengths_bins, effects_ppm, args.trials,
                                    chromosomes=list(args.chromosomes), seed=args.seed, n_depths=len(depths_ppm) if depths_ppm else 1)
    except ValueError as exc:
        print('ERROR:', exc)
        sys.exit(2)
    reference = wt.Reference.from_npz(stored)
    cut = zThreshold([int(v) for v in stored['masked_sizes']], args.multitest, args.minzscore)
    print('z-score threshold per bin:', cut)
    samples = [ingest.read_sample(path, reference.binsize)[0] for path in args.infiles]
    began = time.time()
    rec_i, rec_f = sensitivity.sensitivity_batch(reference, samples, plan, cut, minrefbins=args.minrefbins, repeats=args.repeats,
                                                 chromosomes=list(args.chromosomes), mineffectsize=args.mineffectsize,
                                                 batch=args.batch, depths_ppm=depths_ppm, draw=draw, seed=args.seed)
    print('%d trials took %.3f s' % (len(plan), time.time() - began))
    table = sensitivity.sensitivityTable(plan, rec_i, rec_f, lengths_bins, effects_ppm, minoverlap=args.minoverlap,
                                         depths_ppm=depths_ppm, n_samples=len(args.infiles))
    text = sensitivity.tableText(table)
    npz_path, tsv_path = sensitivityOutputs(args.outfile)
    # (depths_ppm and draw are members only when one of the two options is given: without them the file is what it always was)
    extra = dict(depths_ppm=np.array(depths_ppm if depths_ppm else [1000000], dtype=np.int64),
                 draw=np.bool_(draw)) if depths_ppm or draw else {}
    write_npz(npz_path, arguments=vars(args), runtime=getRuntime(), binsize=binsize, threshold_z=cut,
              samples=np.array([str(p) for p in args.infiles]), lengths_bins=np.array(lengths_bins, dtype=np.int64),
              effects_ppm=np.array(effects_ppm, dtype=np.int64), plan=plan, rec_i=rec_i, rec_f=rec_f, table=table, **extra)
    with open(tsv_path, 'w') as handle:
        handle.write(text)
    print(text, end='')
    reference.close()


# -------------------------------------------------------------------- crossval ----
def crossvalOutputs(outfile):
    """(out.npz, out_samples.tsv, out_windows.tsv) of the `out` argument (a trailing .npz is taken as part of none)."""
    stem = outfile[:-4] if outfile.endswith('.npz') else outfile
    return stem + '.npz', stem + '_samples.tsv', stem + '_windows.tsv'


def crossvalBinsOutput(outfile):
    """out_bins.tsv of the `out` argument: the per-bin table of -robust."""
    return crossvalOutputs(outfile)[0][:-4] + '_bins.tsv'


def crossvalRobustPlan(args):
    """The -robust family of `crossval` as (robust, criteria): criteria is None without -maxspread, else the keyword
    arguments of blacklist.listedBins.  ValueError: -makeblacklist without -maxspread, -maxshift or -mincover without
    -maxspread, a criterion that is no number of its range."""
    given = {name: getattr(args, name) for name in ('maxspread', 'maxshift', 'mincover') if hasattr(args, name)}
    if 'maxspread' not in given:
        if hasattr(args, 'makeblacklist'):
            raise ValueError('-makeblacklist needs -maxspread: which spread is too wide is the cohort\'s to say')
        if given:
            raise ValueError('-%s goes with -maxspread' % sorted(given)[0])
        return hasattr(args, 'robust'), None
    if not given['maxspread'] > 0 or not given.get('maxshift', 1.0) > 0 or not 0 <= given.get('mincover', 0.5) <= 1:
        raise ValueError('-maxspread and -maxshift are above 0 and -mincover lies in 0 .. 1')
    return True, dict(maxspread=given['maxspread'], maxshift=given.get('maxshift'), mincover=given.get('mincover', 0.5))


def crossvalPlan(args):
    """What `crossval` can refuse before the GPU is touched, as ValueError: fewer than 5 files, a bad fold count, bad
    -windows, no chromosome, bin sizes that do not scale.  Returns (fold_of, window lengths, the bin size the files are
    read at)."""
    from . import crossval
    n = len(args.infiles)
    if n < 5:
        raise ValueError('crossval needs 5 healthy samples at least, got %d' % n)
    fold_of = crossval.foldPlan(n, n if args.loo else args.folds, seed=args.seed)
    windows = crossval.parseWindows(args.windows)
    crossvalRobustPlan(args)
    if not args.chromosomes or args.refsize < 1:
        raise ValueError('crossval needs -refsize >= 1 and at least one chromosome')
    if args.results is not None:
        from . import ingest
        ingest.output_names(args.infiles, args.results)        # two inputs with one leaf name would share a result file
    own =[_open_npz(path)['arguments'].item()['binsize'] for path in args.infiles]
    if args.binsize is None:
        if len(set(float(v) for v in own)) > 1:
            raise ValueError('the input samples were binned at different sizes %s: give -binsize to merge them to a common size'
                             % sorted(set(float(v) for v in own)))
        return fold_of, windows, own[0]
    for path, size in zip(args.infiles, own):
        if size == 0 or args.binsize < size or args.binsize % size > 0:
            raise ValueError('%s was binned at %s, which does not scale to -binsize %s' % (path, size, args.binsize))
    return fold_of, windows, args.binsize


def toolCrossval(args):
    """`crossval healthy... out [-folds N | -loo]` (build-only): every healthy sample is tested against a reference built
    from the samples of the other folds, as `newref` builds and `test` tests, and the held-out z-scores of the whole cohort
    are judged on the GPU (crossval.crossval_batch).  Writes out.npz (every array of the run), out_samples.tsv (a line per
    sample: the samples with calls are what to look at) and out_windows.tsv (a line per window length: how often
    sum(z) / sqrt(L) of healthy held-out data passes the threshold, and how wide it is spread); with -results DIR also a
    `test`-format file per held-out sample, DIR/<stem>_test.npz.  Everything that can be refused is refused before the GPU
    is touched: exit status 2.

    -blacklist FILE drops the file's bins from every fold's reference, as `newref -blacklist` does.  -robust adds the per-bin
    median and median absolute deviation of the held-out z-scores (wc_column_robust_dev) to out.npz and writes
    out_bins.tsv; -makeblacklist FILE -maxspread S [-maxshift M] [-mincover C] also writes the bins blacklist.listedBins
    lists as a BED file."""
    from . import crossval
    try:
        fold_of, windows, binsize = crossvalPlan(args)
        robust, criteria = crossvalRobustPlan(args)
    except ValueError as exc:
        print('ERROR:', exc)
        sys.exit(2)
    from . import ingest
    counts, chrom_sizes, _ = ingest.load_counts(args.infiles, args.binsize, threads=min(16, os.cpu_count() or 1), verbose=True)
    try:
        drop = readBlacklistOption(args, chrom_sizes, binsize)
    except (ValueError, OSError) as exc:
        print('ERROR:', exc)
        sys.exit(2)
    extra = dict(drop=drop) if drop is not None else {}
    if robust:
        extra['robust'] = True
    began = time.time()
    result = crossval.crossval_batch(counts, chrom_sizes, fold_of, binsize, refsize=args.refsize, multitest=args.multitest,
                                     minzscore=args.minzscore, minrefbins=args.minrefbins, repeats=args.repeats,
                                     chromosomes=list(args.chromosomes), mineffectsize=args.mineffectsize, windows=windows,
                                     keep_results=args.results is not None, **extra)
    print('%d folds over %d samples took %.3f s' % (int(fold_of.max()) + 1, len(fold_of), time.time() - began))
    npz_path, samples_path, windows_path = crossvalOutputs(args.outfile)
    table = crossval.windowsTable(windows, result['win_n'], result['win_i'], result['win_hist'], result['rec_f'][:, 1])
    stored = {key: value for key, value in result.items() if key not in ('Z', 'R', 'results_cwz')}
    if drop is not None:
        stored['blacklist'] = drop
    write_npz(npz_path, arguments=vars(args), runtime=getRuntime(), binsize=binsize, samples=np.array([str(p) for p in args.infiles]),
              chromosome_sizes=np.array(chrom_sizes, dtype=np.int64), windows=np.array(windows, dtype=np.int64), **stored)
    if robust:
        from . import blacklist
        listed = np.zeros(len(result['robust_i']), dtype=bool)
        if criteria is not None:
            listed = blacklist.listedBins(result['robust_i'], result['robust_f'], len(fold_of), **criteria)
        with open(crossvalBinsOutput(args.outfile), 'w') as handle:
            handle.write(crossval.binsText(chrom_sizes, binsize, result['bins_i'], result['bins_f'], result['robust_f'], listed))
        if hasattr(args, 'makeblacklist'):
            note = ' '.join('%s=%r' % (key, value) for key, value in sorted(criteria.items()) if value is not None)
            runs = blacklist.writeBlacklist(args.makeblacklist, listed, chrom_sizes, binsize, note=note)
            print('Blacklist %s: %d bins in %d runs listed' % (args.makeblacklist, int(listed.sum()), runs))
    with open(samples_path, 'w') as handle:
        handle.write(crossval.samplesText([os.path.basename(str(p)) for p in args.infiles], result['rec_i'], result['rec_f']))
    text = crossval.windowsText(table)
    with open(windows_path, 'w') as handle:
        handle.write(text)
    print(text, end='')
    with_calls = np.flatnonzero(result['rec_i'][:, 1] > 0)
    print('%d of %d held-out samples carry a call%s' % (len(with_calls), len(fold_of),
                                                       ': ' + ', '.join(os.path.basename(str(args.infiles[i])) for i in with_calls)
                                                       if len(with_calls) else ''))
    if args.results is not None:
        os.makedirs(args.results, exist_ok=True)
        names = ingest.output_names(args.infiles, args.results)
        for name, fold, held in zip(names, fold_of, crossval.heldOutResults(result, chrom_sizes)):
            writeTestOutput(name, args, binsize, held, result['threshold'][fold])


# ------------------------------------------------------------------ downsample ----
def toolDownsample(args):
    """`downsample in.npz out.npz (-fraction F | -reads N)` (build-only): a converted sample thinned on the GPU to a
    fraction of its reads, every read kept with probability keep_ppm / 10^6 (sensitivity.thinCounts: chromosome int(key),
    row id 0, the file's own bin size).  -reads N keeps min(10^6, N * 10^6 // total) ppm: the kept total is a draw around
    N, not N.  `arguments` are those of the input plus the options given here, `quality` is copied with the kept total
    under 'downsampled'.  Refusals come before the GPU is touched: exit status 2."""
    from . import sensitivity
    try:
        stored = _open_npz(args.infile)
        sample = stored['sample'].item()
        numbers = {}
        for key in sample:
            try:
                numbers[key] = int(key)
            except ValueError:
                raise ValueError('chromosome key %r is not a number' % (key,))
            if not 1 <= numbers[key] <= 64:
                raise ValueError('chromosome key %r is outside 1 .. 64' % (key,))
        if not numbers:
            raise ValueError('%s holds no chromosome' % args.infile)
        total = int(sum(int(np.asarray(sample[key]).clip(0).sum()) for key in sample))
        if hasattr(args, 'fraction'):
            if not 0 < args.fraction <= 1 or int(round(args.fraction * 1e6)) < 1:
                raise ValueError('-fraction %r is out of range (a fraction in (0, 1] of 1 ppm at least)' % args.fraction)
            keep_ppm = int(round(args.fraction * 1e6))
        else:
            if args.reads < 1 or total < 1:
                raise ValueError('-reads %d of %d reads' % (args.reads, total))
            keep_ppm = min(1000000, (args.reads * 1000000) // total)
            if keep_ppm < 1:
                raise ValueError('-reads %d of %d reads is less than 1 ppm' % (args.reads, total))
    except ValueError as exc:
        print('ERROR:', exc)
        sys.exit(2)
    sizes = np.zeros(max(numbers.values()), dtype=np.int64)
    for key, number in numbers.items():
        sizes[number - 1] = len(sample[key])
    offs = np.concatenate([[0], np.cumsum(sizes)])
    image = np.zeros((1, int(offs[-1])), dtype=np.int32)
    for key, number in numbers.items():
        image[0, offs[number - 1]:offs[number]] = sample[key]
    thinned = sensitivity.thinCounts(image, sizes, [keep_ppm], seed=args.seed)[0, 0]
    out = {key: thinned[offs[number - 1]:offs[number]].astype(np.asarray(sample[key]).dtype) for key, number in numbers.items()}
    arguments = dict(stored['arguments'].item())
    arguments.update({name: value for name, value in vars(args).items() if name in ('fraction', 'reads', 'seed')})
    quality = dict(stored['quality'].item())
    quality['downsampled'] = int(thinned.clip(0).sum())
    write_npz(args.outfile, arguments=arguments, runtime=getRuntime(), sample=out, quality=quality)
    print('kept %d of %d reads (%d ppm)' % (quality['downsampled'], total, keep_ppm))


# ---------------------------------------------------------------------- parser ----
def _not_in_this_build(args):
    print('ERROR: this sub-command is not part of the MI355X build (convert, newref*, test, report, plotbatch only): '
          'plot writes a matplotlib PDF by default, which this build does not make; use plotbatch for PNG files or '
          'run it with the upstream wisecondor.py')
    sys.exit(2)


def _chromosome_list(text):
    return [int(token) for token in text.split(',')]


#: `-blacklist` of newref, newrefprep and crossval (build-only).  SUPPRESS keeps it out of the namespace, and so out of the
#: `arguments` of the written files and of `report`'s text, unless it is given
_BLACKLIST_OPTION = dict(type=str, default=argparse.SUPPRESS,
                         help='BED file (base pairs, chr1 .. chr22 or 1 .. 22) of regions to leave out of the reference: a bin '
                              'that meets one is masked like a bin without reads')

#: options shared by `test` and `testbatch`: (flag, argparse settings)
_TEST_OPTIONS = (
    ('-minzscore', dict(type=float, default=None,
                        help='fixed |z| cut per bin instead of the one derived from -multitest')),
    ('-chromosomes', dict(type=_chromosome_list, default=list(range(1, 23)),
                          help='autosomes to segment, comma separated (default 1..22)')),
    ('-mineffectsize', dict(type=float, default=0,
                            help='ignore windows whose median ratio deviates less than this from 1')),
    ('-multitest', dict(type=float, default=1000,
                        help='number of samples the false-positive budget is spread over')),
    ('-minrefbins', dict(type=int, default=25,
                         help='bins with fewer usable reference bins are left out')),
    ('-repeats', dict(type=int, default=5,
                      help='z-score passes, aberrant bins masked between passes')),
)


def buildParser():
    parser = argparse.ArgumentParser(
        description='WISECONDOR newref / test on AMD MI355X (drop-in for the upstream sub-commands)')
    sub = parser.add_subparsers()

    p = sub.add_parser('plot', description='not provided by this build')
    p.add_argument('rest', nargs=argparse.REMAINDER)
    p.set_defaults(func=_not_in_this_build)

    #: the options `convert` and `convertbatch` share (upstream wisecondor.py:359-367)
    convert_options = (
        ('-binsize', dict(type=float, default=1e6, help='Size per bin in bp')),
        ('-retdist', dict(type=int, default=4,
                          help='Maximum amount of base pairs difference between sequential reads to consider them '
                               'part of the same tower')),
        ('-retthres', dict(type=int, default=4,
                           help='Threshold for when a group of reads is considered a tower and will be removed')),
        # build-only: convertBam's mapq / demandPair, which the upstream command line does not reach.  SUPPRESS keeps them
        # out of the namespace (the `arguments` of the output file, which `report` prints) unless they are given
        ('-mapq', dict(type=int, default=argparse.SUPPRESS,
                       help='Lowest mapping quality of a read that is counted (default 1)')),
        ('-paired', dict(action='store_true', default=argparse.SUPPRESS,
                         help='Paired-end mode: count proper-pair first-in-pair reads only, a duplicate repeats the '
                              'previous read\'s position and mate position')),
        ('-stream', dict(action='store_true', default=argparse.SUPPRESS,
                         help='Read the BAM through the GPU in chunks (memory bounded by the chunk, not the file)')),
        ('-bounded', dict(action='store_true', default=argparse.SUPPRESS,
                          help='Read AND filter the BAM chunk by chunk: no per-read arrays, device memory independent of '
                               'the read count, no limit on the number of reads')),
        ('-chunk', dict(type=int, default=argparse.SUPPRESS,
                        help='Compressed bytes per chunk of -stream / -bounded (default: the library\'s)')),
    )
    p = sub.add_parser('convert', description='Convert and filter a bam file to an npz')
    p.add_argument('infile', type=str, help='Bam input file for conversion')
    p.add_argument('outfile', type=str, help='File to write binned information to')
    for flag, settings in convert_options:
        p.add_argument(flag, **settings)
    p.set_defaults(func=toolConvert)

    p = sub.add_parser('convertbatch', description='convert for many bam files, file work overlapped (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='Bam input files')
    p.add_argument('outdir', type=str, help='directory receiving <name>.npz per bam file')
    p.add_argument('-io', type=int, default=8, help='threads that inflate a bam file')
    for flag, settings in convert_options:
        p.add_argument(flag, **settings)
    p.set_defaults(func=toolConvertBatch)

    p = sub.add_parser('report', description='Print the text summary of a converted sample and its test result')
    p.add_argument('testfile', type=str, help='converted sample (.npz) the test was run on')
    p.add_argument('resultfile', type=str, help='result file written by test')
    p.add_argument('-mineffect', type=float, default=1.5,
                   help='Minimal percentual change in read depth of a call to report')
    p.set_defaults(func=toolReport)

    p = sub.add_parser('plotbatch', description='z-score panel PNGs of many result files, drawn on the GPU (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='result files written by test / testbatch (.npz)')
    p.add_argument('outdir', type=str, help='directory receiving <name>_z.png per result file')
    # the first five as upstream plot (wisecondor.py:460-479)
    p.add_argument('-cytofile', type=str, default=None, help='File containing cytoband information')
    p.add_argument('-chromosomes', type=_chromosome_list, default=list(range(1, 23)),
                   help='Integer representation of chromosomes to plot, comma separated (default 1..22)')
    p.add_argument('-columns', type=int, default=2, help='Amount of columns to distribute plots over')
    p.add_argument('-size', type=float, nargs=2, default=[11.7, 8.3], help='Size of plot in inches, default is A4 landscape')
    p.add_argument('-mineffect', type=float, default=1.5, help='Minimal percentual change in read depth of a call to plot')
    p.add_argument('-filetype', type=str, default='png', help='png only')
    p.add_argument('-dpi', type=int, default=100, help='pixels per inch')
    p.add_argument('-batch', type=int, default=64, help='images per GPU batch')
    p.add_argument('-io', type=int, default=8, help='file read / write threads')
    p.set_defaults(func=toolPlotBatch)

    p = sub.add_parser('plotpdf', description='z-score panel PDFs (vector) of many result files, written on the GPU (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='result files written by test / testbatch (.npz)')
    p.add_argument('outdir', type=str, help='directory receiving <name>_z.pdf per result file')
    # the five options of upstream plot (wisecondor.py:460-479), with its defaults
    p.add_argument('-cytofile', type=str, default=None, help='File containing cytoband information')
    p.add_argument('-chromosomes', type=_chromosome_list, default=list(range(1, 23)),
                   help='Integer representation of chromosomes to plot, comma separated (default 1..22)')
    p.add_argument('-columns', type=int, default=2, help='Amount of columns to distribute plots over')
    p.add_argument('-size', type=float, nargs=2, default=[11.7, 8.3], help='Size of plot in inches, default is A4 landscape')
    p.add_argument('-mineffect', type=float, default=1.5, help='Minimal percentual change in read depth of a call to plot')
    p.add_argument('-batch', type=int, default=64, help='pages per GPU batch')
    p.add_argument('-io', type=int, default=8, help='file read / write threads')
    p.set_defaults(func=toolPlotPdf)

    p = sub.add_parser('exportjson', description='result files as lossless JSON, the digits made on the GPU (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='result files written by test / testbatch (.npz)')
    p.add_argument('outdir', type=str, help='directory receiving <name>.json per result file')
    p.add_argument('-strict', action='store_true', help='write null for Infinity, -Infinity and NaN (strict JSON)')
    p.add_argument('-gz', action='store_true', help='write <name>.json.gz, the arrays deflated on the GPU')
    p.add_argument('-batch', type=int, default=64, help='files per GPU batch')
    p.add_argument('-io', type=int, default=8, help='file read / write threads')
    p.set_defaults(func=toolExportJson)

    p = sub.add_parser('exporttracks', description='result files as bedGraph tracks and BED calls for genome browsers, '
                                                   'text and BGZF made on the GPU (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='result files written by test / testbatch (.npz)')
    p.add_argument('outdir', type=str, help='directory receiving <name>_z.bedgraph, <name>_r.bedgraph and <name>_calls.bed per result file')
    p.add_argument('-gz', action='store_true', help='write the tracks as <name>_z.bedgraph.gz / _r.bedgraph.gz (BGZF, made on the GPU)')
    p.add_argument('-nozero', action='store_true', help='leave out runs of 0.0 (the fill of masked bins) as well as those not finite')
    p.add_argument('-only', choices=('z', 'r'), default=None, help='write one of the two tracks')
    p.add_argument('-chrprefix', type=str, default='chr', help='chromosome i is named <prefix>i (may be empty, at most 16 bytes)')
    p.add_argument('-chromsizes', type=str, default=None, help='name<TAB>length file; ends are clipped to the lengths')
    p.add_argument('-mineffect', type=float, default=0, help='Minimal percentual change in read depth of a call to export')
    p.add_argument('-batch', type=int, default=64, help='files per GPU batch')
    p.add_argument('-io', type=int, default=8, help='file read / write threads')
    p.set_defaults(func=toolExportTracks)

    p = sub.add_parser('newref', description='Build a reference from healthy samples in one go')
    p.add_argument('infiles', type=str, nargs='*', help='converted reference samples (.npz)')
    p.add_argument('outfile', type=str, help='reference file to write (.npz)')
    p.add_argument('-refsize', type=int, default=100, help='reference bins kept per target bin')
    p.add_argument('-binsize', type=int, default=None,
                   help='merge sample bins to this size first (a multiple of their own size)')
    p.add_argument('-cpus', type=int, default=1,
                   help='upstream worker count: sets the number of part files and, up to the '
                        'number of visible GPUs, of GPU processes')
    p.add_argument('-parts', type=int, default=1, help='number of part files when larger than -cpus')
    p.add_argument('-gpus', type=int, default=None, help='GPU processes to use (build-only option)')
    p.add_argument('-blacklist', **_BLACKLIST_OPTION)
    p.set_defaults(func=toolNewref)

    p = sub.add_parser('newrefprep', description='Step 1 of a split reference build: the prep file')
    p.add_argument('infiles', type=str, nargs='*', help='converted reference samples (.npz)')
    p.add_argument('prepfile', type=str, help='prep file to write (.npz)')
    p.add_argument('-binsize', type=int, default=None,
                   help='merge sample bins to this size first (a multiple of their own size)')
    p.add_argument('-blacklist', **_BLACKLIST_OPTION)
    p.set_defaults(func=toolNewrefPrep)

    p = sub.add_parser('newrefpart', description='Step 2 of a split reference build: one part')
    p.add_argument('prepfile', type=str, help='prep file of step 1')
    p.add_argument('partfile', type=str, help='base name of the part files; _<m>.npz is appended')
    p.add_argument('part', type=int, default=[0, 1], nargs=2, help='m n: compute part m of n')
    p.add_argument('-refsize', type=int, default=100, help='reference bins kept per target bin')
    p.set_defaults(func=toolNewrefPart)

    p = sub.add_parser('newrefpost', description='Step 3 of a split reference build: the merge')
    p.add_argument('prepfile', type=str, help='prep file of step 1')
    p.add_argument('partfile', type=str, help='base name of the part files of step 2')
    p.add_argument('parts', type=int, default=1, help='how many parts step 2 was split into')
    p.add_argument('outfile', type=str, help='reference file to write (.npz)')
    p.set_defaults(func=toolNewrefPost)

    p = sub.add_parser('test', description='Call copy number aberrations in one sample')
    p.add_argument('infile', type=str, help='converted sample (.npz)')
    p.add_argument('outfile', type=str, help='result file to write (.npz)')
    p.add_argument('reference', type=str, help='reference built by newref')
    for flag, settings in _TEST_OPTIONS:
        p.add_argument(flag, **settings)
    p.set_defaults(func=toolTest)

    p = sub.add_parser('testbatch', description='test for many samples per GPU batch (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='converted samples (.npz)')
    p.add_argument('outdir', type=str, help='directory receiving <sample>_test.npz')
    p.add_argument('reference', type=str, help='reference built by newref')
    p.add_argument('-batch', type=int, default=256, help='samples per GPU batch')
    p.add_argument('-gpus', type=int, default=None, help='GPU processes to shard the samples over')
    p.add_argument('-io', type=int, default=8, help='file decode / encode threads')
    p.add_argument('-ziplevel', type=int, default=1,
                   help='zlib level of the result files (0 = stored, 1 = run-length deflate: the same size at a third of '
                        'the time on these arrays, 6 = what np.savez_compressed uses)')
    # build-only; SUPPRESS keeps it out of the namespace (and the `arguments` of the result files) unless it is given
    p.add_argument('-encoder', choices=('host', 'gpu'), default=argparse.SUPPRESS,
                   help='who deflates results_z / results_r: the I/O threads (host, the default) or the GPU, from which '
                        'then only the compressed streams are copied (gpu; goes with -ziplevel 1 only)')
    for flag, settings in _TEST_OPTIONS:
        p.add_argument(flag, **settings)
    p.set_defaults(func=toolTestBatch)

    p = sub.add_parser('sensitivity', description='plant aberrations into healthy samples on the GPU and count how often the '
                                                  'reference finds them (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='converted healthy samples (.npz)')
    p.add_argument('outfile', type=str, help='out: out.npz (plan, records, table) and out.tsv (table) are written')
    p.add_argument('reference', type=str, help='reference built by newref')
    p.add_argument('-lengths', type=str, required=True, help='span lengths in bp, comma separated (1e6,5e6,20e6)')
    p.add_argument('-effects', type=str, required=True,
                   help='changes in read depth in percent, comma separated, -100 .. 10000 (2.5,5,10,-2.5,-5,-10); a list that '
                        'begins with a negative value is written -effects=-5,5')
    p.add_argument('-trials', type=int, default=20, help='placements per sample and length')
    p.add_argument('-seed', type=int, default=1, help='seed of the placements, and the key of the draws of -depths and -draw')
    # build-only additions; SUPPRESS keeps them out of the namespace (and the `arguments` of out.npz) unless they are given
    p.add_argument('-depths', type=str, default=argparse.SUPPRESS,
                   help='fractions of the read depth in (0, 1], comma separated, at most 8 (1,0.5,0.25): the samples are thinned '
                        'on the GPU to each and the grid runs at every depth')
    p.add_argument('-draw', action='store_true', default=argparse.SUPPRESS,
                   help='plant Binomial spikes (a real aberration\'s sampling noise) instead of the rounded product')
    p.add_argument('-minoverlap', type=float, default=0.5,
                   help='a trial counts as detected when its matching calls cover this share of the span')
    p.add_argument('-batch', type=int, default=1024, help='trials per GPU batch')
    for flag, settings in _TEST_OPTIONS:
        p.add_argument(flag, **settings)
    p.set_defaults(func=toolSensitivity)

    p = sub.add_parser('crossval', description='test every healthy sample against a reference built without its fold and judge the '
                                               'held-out z-scores on the GPU (build-only)')
    p.add_argument('infiles', type=str, nargs='+', help='converted healthy samples (.npz), 5 at least')
    p.add_argument('outfile', type=str, help='out: out.npz, out_samples.tsv and out_windows.tsv are written')
    how = p.add_mutually_exclusive_group()
    how.add_argument('-folds', type=int, default=10, help='folds of the cohort (default 10)')
    how.add_argument('-loo', action='store_true', help='leave one out: as many folds as files')
    p.add_argument('-seed', type=int, default=1, help='seed of the fold plan')
    p.add_argument('-refsize', type=int, default=100, help='reference bins kept per target bin')
    p.add_argument('-binsize', type=int, default=None,
                   help='merge sample bins to this size first (a multiple of their own size)')
    p.add_argument('-windows', type=str, default='1,2,5,10,20,50,100',
                   help='window lengths in bins, comma separated, ascending, at most 16')
    p.add_argument('-results', type=str, default=None,
                   help='directory receiving <sample>_test.npz, the held-out result of every sample in the format of test')
    for flag, settings in _TEST_OPTIONS:
        p.add_argument(flag, **settings)
    p.add_argument('-blacklist', **_BLACKLIST_OPTION)
    # build-only additions; SUPPRESS keeps them out of the namespace (and the `arguments` of out.npz) unless they are given
    p.add_argument('-robust', action='store_true', default=argparse.SUPPRESS,
                   help='per bin the median and the median absolute deviation of the held-out z-scores, from the GPU: two more '
                        'arrays in out.npz, and out_bins.tsv')
    p.add_argument('-makeblacklist', type=str, default=argparse.SUPPRESS,
                   help='BED file to write: the bins whose robust spread lies above -maxspread (implies -robust, needs -maxspread)')
    p.add_argument('-maxspread', type=float, default=argparse.SUPPRESS, help='list a bin when 1.4826 * mad of its z-scores is above this')
    p.add_argument('-maxshift', type=float, default=argparse.SUPPRESS, help='and when the |median| of its z-scores is above this')
    p.add_argument('-mincover', type=float, default=argparse.SUPPRESS,
                   help='but only bins that this share of the samples tested with a finite z (default 0.5)')
    p.set_defaults(func=toolCrossval)

    p = sub.add_parser('downsample', description='thin a converted sample to a fraction of its reads on the GPU (build-only)')
    p.add_argument('infile', type=str, help='converted sample (.npz)')
    p.add_argument('outfile', type=str, help='thinned sample to write (.npz)')
    how = p.add_mutually_exclusive_group(required=True)
    how.add_argument('-fraction', type=float, default=argparse.SUPPRESS, help='keep every read with this probability, in (0, 1]')
    how.add_argument('-reads', type=int, default=argparse.SUPPRESS,
                     help='keep every read with probability N / (the file\'s reads), in whole ppm: the kept total is a draw around N, '
                          'not N')
    p.add_argument('-seed', type=int, default=1, help='key of the draws')
    p.set_defaults(func=toolDownsample)
    return parser


def main(argv=None):
    parser = buildParser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if not hasattr(args, 'func'):
        parser.print_usage()
        sys.exit(2)
    printArgs(args)
    args.func(args)


if __name__ == '__main__':
    main()
