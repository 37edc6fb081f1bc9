"""Host-side mirror of the reference's wisetools.py for the newref / test hot path.

Same function names, argument meaning and return shapes as the upstream
functions (cited per function as wisetools.py:line), but every numeric step
runs in the gfx950 HIP library through the C ABI (include/wisecondor_hip.h).
No numpy fallback exists: without the library or a GPU these functions raise.
"""
import ctypes
import os

import numpy as np

from . import _lib

SENTINEL_INDEX = -1
SENTINEL_DISTANCE = 1e10


def getPart(partnum, outof, bincount):
    """Rows [start, end) of zero-based part `partnum` (wisetools.py:358-361)."""
    a, b = ctypes.c_int64(), ctypes.c_int64()
    _lib.load().wc_get_part(int(partnum), int(outof), int(bincount), ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def sum_order_of(correctedData):
    """Rounding order numpy would use for np.sum(..., 1) on this array (wisetools.py:302).

    numpy reduces along the smaller-stride axis in its inner loop: a C-ordered
    [bins, samples] array gets a pairwise sum per row, the Fortran-ordered array
    np.load returns for a prep file (trainPCA's corrected.T, wisetools.py:101) a
    plain sample-by-sample sum.  The HIP library reproduces either.
    """
    a = np.asarray(correctedData)
    if a.ndim != 2 or a.shape[1] <= 1 or a.flags["C_CONTIGUOUS"]:
        return _lib.SUM_PAIRWISE
    return _lib.SUM_PAIRWISE if abs(a.strides[1]) <= abs(a.strides[0]) else _lib.SUM_SEQUENTIAL


def getReference(correctedData, chromosomeBins, chromosomeBinSums, selectRefAmount=100, part=1,
                 splitParts=1, device=0):
    """Reference bins for the rows of part `part` of `splitParts` (wisetools.py:364-398).

    Returns (int32 [rows, k] positions in the other-chromosomes concatenation,
    float64 [rows, k] ascending squared distances), -1 / 1e10 padded.
    """
    lib = _lib.load()
    ctx = _lib.context(device)
    order = sum_order_of(correctedData)
    data = np.ascontiguousarray(correctedData, dtype=np.float64)
    bins = np.ascontiguousarray(chromosomeBins, dtype=np.int64)
    n_bins = int(np.asarray(chromosomeBinSums)[-1])
    if data.ndim != 2 or data.shape[0] != n_bins:
        raise ValueError("correctedData must be [bins, samples] with %d bins" % n_bins)
    start, end = getPart(part - 1, splitParts, n_bins)
    print('Working on part', part, 'of', splitParts, 'meaning bins', start, 'up to', end)
    k = int(selectRefAmount)
    rows = max(end - start, 0)
    idx = np.empty((rows, k), dtype=np.int32)
    dst = np.empty((rows, k), dtype=np.float64)
    _lib.check(lib.wc_get_reference(ctx, _lib.ptr(data), n_bins, data.shape[1], _lib.ptr(bins),
                                    bins.shape[0], k, order, start, end, _lib.ptr(idx), _lib.ptr(dst)))
    return idx, dst


def newref_stats(device=0):
    """Counters of the last getReference call on this device (see wc_newref_stats)."""
    out = np.zeros(8, dtype=np.int64)
    _lib.check(_lib.load().wc_newref_stats(_lib.context(device), _lib.ptr(out)))
    return dict(fast_rows=int(out[0]), fallback_rows=int(out[1]), tiles=int(out[2]),
                sample_cols=int(out[3]), rescored=int(out[4]))


# ---------------------------------------------------------------------------
# test path
# ---------------------------------------------------------------------------
MAX_CALLS = 256  # per sample (and per region) capacity handed to the C ABI


def scaleSample(sample, fromSize, toSize):
    """Merge bins to a coarser size (wisetools.py:220-237); host data marshalling."""
    if fromSize == toSize or toSize is None:
        return sample
    if toSize == 0 or fromSize == 0 or toSize < fromSize or toSize % fromSize > 0:
        print('ERROR: Impossible binsize scaling requested:', fromSize, 'to', toSize)
        raise SystemExit(1)
    scale = int(toSize / fromSize)
    out = dict()
    for chrom in sample:
        data = np.asarray(sample[chrom])
        new_len = int(np.ceil(len(data) / float(scale)))
        padded = np.zeros(new_len * scale, dtype=np.int64)
        padded[:len(data)] = data
        out[chrom] = padded.reshape(new_len, scale).sum(axis=1).astype(np.int32)
    return out


def samples_to_counts(samples, chromosome_sizes):
    """Dense int32 [n_samples, sum(chromosome_sizes)] image of sample dicts.

    The pad/truncate-to-reference-length part of toNumpyRefFormat
    (wisetools.py:268-274); the arithmetic happens on the GPU.
    """
    sizes = [int(v) for v in chromosome_sizes]
    out = np.zeros((len(samples), int(sum(sizes))), dtype=np.int32)
    for row, sample in enumerate(samples):
        at = 0
        for chrom, want in enumerate(sizes, start=1):
            data = np.asarray(sample[str(chrom)])
            have = min(want, len(data))
            out[row, at:at + have] = data[:have]
            at += want
    return out


class Reference(object):
    """Device-resident reference (`newref` output) shared by every sample of a batch.

    Holds what toolTest derives from the reference file alone
    (wisecondor.py:177-201): the arrays themselves, getOptimalCutoff and the
    per-bin reference lists.
    """

    def __init__(self, indexes, distances, chromosome_sizes, masked_sizes, mask, pca_mean,
                 pca_components, binsize=None, cutoff=None, device=0, ctx=None):
        lib = _lib.load()
        self.device = device
        self.ctx = ctx if ctx is not None else _lib.context(device)     # ctx: a context of _lib.new_context
        self.binsize = binsize
        self.indexes = np.ascontiguousarray(indexes, dtype=np.int32)
        self.distances = np.ascontiguousarray(distances, dtype=np.float64)
        self.chromosome_sizes = np.ascontiguousarray(chromosome_sizes, dtype=np.int64)
        self.masked_sizes = np.ascontiguousarray(masked_sizes, dtype=np.int64)
        self.mask = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
        self.pca_mean = np.ascontiguousarray(pca_mean, dtype=np.float64)
        comps = np.ascontiguousarray(pca_components, dtype=np.float64)
        self.pca_components = comps.reshape(-1, self.pca_mean.shape[0]) if comps.size else comps.reshape(0, self.pca_mean.shape[0])
        self.n_bins, self.k = self.indexes.shape
        self.n_total = int(self.chromosome_sizes.sum())
        override = None
        if cutoff is not None:
            override = ctypes.byref(ctypes.c_double(float(cutoff)))
        self.handle = lib.wc_reference_create(
            self.ctx, _lib.ptr(self.indexes), _lib.ptr(self.distances), self.n_bins, self.k,
            _lib.ptr(self.chromosome_sizes), _lib.ptr(self.masked_sizes), len(self.chromosome_sizes),
            _lib.ptr(self.mask), _lib.ptr(self.pca_mean), _lib.ptr(self.pca_components),
            self.pca_components.shape[0], 3, override)
        if not self.handle:
            raise _lib.WisecondorHipError("wc_reference_create: " + lib.wc_last_error().decode())
        self.cutoff = lib.wc_reference_cutoff(self.handle)

    @classmethod
    def from_npz(cls, npz, device=0):
        binsize = npz['binsize'].item() if hasattr(npz['binsize'], 'item') else npz['binsize']
        return cls(npz['indexes'], npz['distances'], npz['chromosome_sizes'], npz['masked_sizes'],
                   npz['mask'], npz['pca_mean'], npz['pca_components'], binsize=binsize, device=device)

    def clone(self, ctx):
        """The same reference in another context of the same device (its own device copy and user lists)."""
        return Reference(self.indexes, self.distances, self.chromosome_sizes, self.masked_sizes, self.mask,
                         self.pca_mean, self.pca_components, binsize=self.binsize, cutoff=self.cutoff,
                         device=self.device, ctx=ctx)

    def close(self):
        if getattr(self, "handle", None):
            _lib.load().wc_reference_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def toNumpyRefFormat(sample, chromBins, mask, device=0):
    """Pad/truncate, normalise to unit sum, apply the mask (wisetools.py:267-278)."""
    counts = samples_to_counts([sample], chromBins)
    mask = np.asarray(mask).astype(bool)
    n_bins = int(mask.sum())
    # a reference with only the layout (no neighbours, no PCA components) drives the kernels
    sizes = np.asarray(chromBins, dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    msz = np.array([int(mask[offs[i]:offs[i + 1]].sum()) for i in range(len(sizes))], dtype=np.int64)
    ref = Reference(np.zeros((n_bins, 1), np.int32), np.full((n_bins, 1), 1e10), sizes, msz, mask,
                    np.ones(n_bins), np.zeros((0, n_bins)), cutoff=0.0, device=device)
    out = np.empty((1, n_bins))
    raw = np.empty((1, n_bins))
    _lib.check(_lib.load().wc_prepare_samples(ref.ctx, ref.handle, _lib.ptr(counts), 1, _lib.ptr(out), _lib.ptr(raw)))
    ref.close()
    return raw[0]


def applyPCA(sampleData, mean, components, device=0):
    """x / reconstruction from the stored components (wisetools.py:104-113)."""
    x = np.ascontiguousarray(np.atleast_2d(sampleData), dtype=np.float64)
    mean = np.ascontiguousarray(mean, dtype=np.float64)
    comps = np.ascontiguousarray(components, dtype=np.float64).reshape(-1, mean.shape[0])
    out = np.empty_like(x)
    _lib.check(_lib.load().wc_apply_pca(_lib.context(device), _lib.ptr(x), x.shape[0], x.shape[1],
                                        _lib.ptr(mean), _lib.ptr(comps), comps.shape[0], _lib.ptr(out)))
    return out[0] if np.ndim(sampleData) == 1 else out


def getOptimalCutoff(reference, repeats, device=0):
    """Iterated mean + 3 sd clip of the reference distances (wisetools.py:328-336)."""
    d = np.ascontiguousarray(reference, dtype=np.float64)
    if int(repeats) <= 0:       # the loop body never runs: +inf and the float zeros of wisetools.py:330
        return float("inf"), np.zeros(np.shape(reference))
    cutoff = ctypes.c_double()
    # the mask is the LAST iteration's, i.e. against the cutoff of the iteration before (wisetools.py:332)
    mask = np.empty(d.shape, dtype=np.uint8)
    _lib.check(_lib.load().wc_optimal_cutoff_mask(_lib.context(device), _lib.ptr(d), d.size, int(repeats),
                                                  ctypes.byref(cutoff), _lib.ptr(mask)))
    return cutoff.value, mask.view(np.bool_).reshape(np.shape(reference))


def repeatTest(testData, indexes, distances, chromosomeBins, chromosomeBinSums, cutoff, threshold,
               repeats, device=0, reference=None):
    """`repeats` z-score passes with flagging (wisetools.py:438-448).

    testData may be one vector [bins] or a batch [samples, bins]; returns
    (Z, R, refSizes, stdDevAvg) shaped like the input.
    """
    data = np.ascontiguousarray(np.atleast_2d(testData), dtype=np.float64)
    own = reference is None
    if own:
        sizes = np.asarray(chromosomeBins, dtype=np.int64)
        n_bins = int(sizes.sum())
        reference = Reference(indexes, distances, sizes, sizes, np.ones(n_bins, np.uint8), np.zeros(n_bins),
                              np.zeros((0, n_bins)), cutoff=cutoff, device=device)
    z = np.empty_like(data)
    r = np.empty_like(data)
    n = np.empty_like(data)
    sd = np.empty(data.shape[0])
    _lib.check(_lib.load().wc_repeat_test(reference.ctx, reference.handle, _lib.ptr(data), data.shape[0],
                                          float(threshold), int(repeats), _lib.ptr(z), _lib.ptr(r),
                                          _lib.ptr(n), _lib.ptr(sd)))
    if own:
        reference.close()
    if np.ndim(testData) == 1:
        return z[0], r[0], n[0], sd[0]
    return z, r, n, sd


def stdDevAvg(stdDevs, device=0, return_serial_count=False):
    """Mean of the non-NaN standard deviations, added bin by bin like trySample's Python loop
    (wisetools.py:428-435).  stdDevs: [bins] or [samples, bins]."""
    sd = np.ascontiguousarray(np.atleast_2d(stdDevs), dtype=np.float64)
    out = np.empty(sd.shape[0])
    serial = ctypes.c_int32(0)
    _lib.check(_lib.load().wc_std_dev_avg(_lib.context(device), _lib.ptr(sd), sd.shape[0], sd.shape[1],
                                          _lib.ptr(out), ctypes.byref(serial)))
    res = out[0] if np.ndim(stdDevs) == 1 else out
    return (res, serial.value) if return_serial_count else res


def stouffer_segments(regions, threshold, min_search=3, device=0, ratios=None, mineffectsize=0):
    """fillTri / fillTriMin + segmentTri for a list of 1-D z arrays
    (wisetools.py:466-487, triarray.py:59-84).

    With mineffectsize != 0, `ratios` (same shapes as `regions`) drive fillTriMin's
    median filter.  Returns (whole_region_z [n], [[(value, (x, y)), ...] per region]).
    """
    lib = _lib.load()
    regions = [np.ascontiguousarray(r, dtype=np.float64) for r in regions]
    offs = np.zeros(len(regions) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([r.shape[0] for r in regions])
    z = np.ascontiguousarray(np.concatenate(regions) if regions else np.zeros(0))
    if z.size == 0:
        z = np.zeros(1)
    rat = None
    if mineffectsize != 0:
        if ratios is None or [len(r) for r in ratios] != [len(r) for r in regions]:
            raise ValueError("mineffectsize needs one ratio array per region")
        rat = np.ascontiguousarray(np.concatenate([np.asarray(r, dtype=np.float64) for r in ratios])
                                   if regions else np.zeros(1))
        if rat.size == 0:
            rat = np.zeros(1)
    nreg = len(regions)
    whole = np.empty(nreg)
    ncalls = np.zeros(nreg, dtype=np.int32)
    val = np.zeros((nreg, MAX_CALLS))
    cx = np.zeros((nreg, MAX_CALLS), dtype=np.int32)
    cy = np.zeros((nreg, MAX_CALLS), dtype=np.int32)
    _lib.check(lib.wc_stouffer_segments(_lib.context(device), _lib.ptr(z), _lib.ptr(rat), float(mineffectsize),
                                        _lib.ptr(offs), nreg, float(threshold), int(min_search), MAX_CALLS,
                                        _lib.ptr(whole), _lib.ptr(ncalls), _lib.ptr(val), _lib.ptr(cx),
                                        _lib.ptr(cy)))
    segs = [[(val[r, c], (int(cx[r, c]), int(cy[r, c]))) for c in range(ncalls[r])] for r in range(nreg)]
    return whole, segs


def fillTri(region, device=0):
    """Window triangle of a region (wisetools.py:466-472), never materialised on the GPU."""
    from .triarray import TriArr
    return TriArr.from_region(region, device=device)


def fillTriMin(regionZ, regionR, threshold, device=0):
    """fillTri, or its median-effect filtered variant when threshold != 0 (wisetools.py:475-487)."""
    from .triarray import TriArr
    if threshold == 0:
        return fillTri(regionZ, device=device)
    return TriArr.from_region(regionZ, device=device, ratio=regionR, mineffectsize=threshold)


def inflateArray(array, mask):
    """Scatter into the True positions of mask (wisetools.py:281-288); host shaping helper."""
    mask = np.asarray(mask)
    temp = np.zeros(mask.shape[0])
    temp[np.flatnonzero(mask)] = array
    return temp


def inflateArrayMulti(array, mask_list):
    """wisetools.py:291-295."""
    temp = array
    for mask in reversed(mask_list):
        temp = inflateArray(temp, mask)
    return temp


def test_batch(reference, samples, threshold, minrefbins=25, repeats=5, chromosomes=None, mineffectsize=0):
    """Numeric content of toolTest (wisecondor.py:199-268) for a list of sample dicts.

    Returns a list of dicts with results_z / results_r (per-chromosome lists),
    results_cwz, results_calls, asdef.  Samples must already be at the
    reference's bin size (see scaleSample).
    """
    lib = _lib.load()
    if chromosomes is None:
        chromosomes = list(range(1, 23))
    sel = np.ascontiguousarray(chromosomes, dtype=np.int32)
    out = []
    max_batch = max(1, 60000 // max(1, len(sel)))
    sizes = [int(v) for v in reference.chromosome_sizes]
    for lo in range(0, len(samples), max_batch):
        chunk = samples[lo:lo + max_batch]
        counts = samples_to_counts(chunk, sizes)
        ns = counts.shape[0]
        rz = np.empty((ns, reference.n_total))
        rr = np.empty((ns, reference.n_total))
        cwz = np.empty((ns, max(len(sel), 1)))
        ncalls = np.zeros(ns, dtype=np.int32)
        asdef = np.empty(ns)
        # The reference has no limit on the number of calls; the library's output arrays have one
        # (max_calls per sample and chromosome).  A sample that exceeds it -- e.g. one with almost
        # no reads -- is simply run again with more room.
        max_calls = MAX_CALLS
        while True:
            calls = np.zeros((ns, max_calls, 5))
            rc = lib.wc_test_batch(reference.ctx, reference.handle, _lib.ptr(counts), ns, float(threshold),
                                   int(minrefbins), int(repeats), float(mineffectsize), _lib.ptr(sel), len(sel),
                                   max_calls, _lib.ptr(rz), _lib.ptr(rr), _lib.ptr(cwz), _lib.ptr(calls),
                                   _lib.ptr(ncalls), _lib.ptr(asdef))
            if rc == _lib.E_LIMIT and b"max_calls" in lib.wc_last_error() and max_calls < reference.n_total:
                max_calls *= 4
                continue
            _lib.check(rc)
            break
        offs = np.concatenate([[0], np.cumsum(sizes)])
        for i in range(ns):
            out.append(dict(
                results_z=[rz[i, offs[c]:offs[c + 1]].copy() for c in range(len(sizes))],
                results_r=[rr[i, offs[c]:offs[c + 1]].copy() for c in range(len(sizes))],
                results_cwz=cwz[i, :len(sel)].copy(),
                results_calls=calls[i, :ncalls[i]].copy(),
                asdef=float(asdef[i])))
    return out


# ---------------------------------------------------------------------------
# newref prep (upstream of the hot path)
# ---------------------------------------------------------------------------
def _leading_eigenpairs(gram, n):
    """The n largest eigenvalues (descending) and unit eigenvectors (rows) of the symmetric `gram`
    on the host (LAPACK): the route of WC_PREP_EIG=host and of matrices eigh.hip does not take."""
    n_s = gram.shape[0]
    try:
        from scipy.linalg import eigh as _eigh          # LAPACK dsyevr on the wanted pairs only
        vals, vecs = _eigh(gram, subset_by_index=(max(0, n_s - n), n_s - 1), driver='evr')
    except Exception:                                    # no scipy: numpy's full decomposition
        vals, vecs = np.linalg.eigh(gram)
    order = np.argsort(vals)[::-1][:n]
    return np.ascontiguousarray(vals[order]), np.ascontiguousarray(vecs[:, order].T)


EIG_ON_GPU_FROM = 3         # samples: every size the solver takes stays on the GPU (up to 128 samples the whole
                            # tridiagonalisation is ONE workgroup with the matrix in LDS; LAPACK on the fetched Gram
                            # matrix is ~0.25 ms quicker at 100 samples: WC_PREP_EIG=host)


def _eig_on_gpu(n_s, pcacomp):
    """Where trainPCA's [samples, samples] eigenproblem is solved: WC_PREP_EIG=gpu|host, else by size."""
    mode = os.environ.get('WC_PREP_EIG', 'auto')
    if mode not in ('auto', 'gpu', 'host'):
        raise ValueError("WC_PREP_EIG must be gpu, host or auto, not %r" % mode)
    possible = 3 <= n_s <= 4096 and 1 <= pcacomp <= 8
    if mode == 'gpu' and not possible:
        raise ValueError("WC_PREP_EIG=gpu: the GPU solver takes 3..4096 samples and up to 8 components")
    return possible and (mode == 'gpu' or (mode == 'auto' and n_s >= EIG_ON_GPU_FROM))


def sym_eigh_leading(matrix, n_pairs, device=0):
    """The n_pairs largest eigenvalues (descending) and unit eigenvectors (rows) of a symmetric
    float64 matrix by the GPU solver of csrc/eigh.hip.  `matrix`: numpy array or CUDA tensor."""
    import torch
    lib = _lib.load()
    ctx = _lib.context(device)
    m = matrix if isinstance(matrix, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(matrix, dtype=np.float64))
    m = m.to(device=torch.device('cuda', device), dtype=torch.float64).contiguous()
    n = m.shape[0]
    vals = np.empty(n_pairs)
    vecs = np.empty((n_pairs, n))
    torch.cuda.current_stream(device).synchronize()
    _lib.check(lib.wc_sym_eigh_leading_dev(ctx, ctypes.c_void_p(m.data_ptr()), n, int(n_pairs), _lib.ptr(vals),
                                           _lib.ptr(vecs)))
    return vals, vecs


def _pinned(shape):
    """float64 host array in page-locked memory (a device-to-host copy into it runs at the link's
    rate, several times the pageable rate); plain numpy when torch cannot pin."""
    try:
        import torch
        return torch.empty(shape, dtype=torch.float64, pin_memory=True).numpy()   # the array keeps the tensor alive
    except Exception:
        return np.empty(shape)


def prepReference(samples, pcacomp=3, device=0, device_out=False, counts=None, chrom_bins=None, drop=None):
    """toNumpyArray + trainPCA (wisetools.py:240-264, 89-101) with the bins-sized work on the GPU.

    The Gram matrix of the centred [samples, bins] data comes from the GPU (float64 matrix
    cores); its small [samples, samples] eigenproblem is solved for the leading pairs by the direct
    solver of csrc/eigh.hip (from EIG_ON_GPU_FROM samples; below that, and under WC_PREP_EIG=host,
    by LAPACK on the fetched matrix), and the GPU finishes (components, projection,
    reconstruction, division).  Returns
    (maskedData [B,S], chromosomeBins, mask, correctedData [B,S] Fortran-ordered like the
    reference's, pca_components [n,B], pca_mean [B], maskedChromBins).

    device_out=True keeps the two bins x samples matrices in HBM: maskedData and correctedData
    come back as torch tensors on the device, correctedData as the C-ordered [B,S] tensor that
    getReference / NewrefJob take directly -- its values are those of the reference's
    Fortran-ordered array, so pass sum_order=_lib.SUM_SEQUENTIAL.

    counts / chrom_bins: the samples already as the dense int32 [samples, bins] matrix of
    samples_to_counts (a caller that ingests many files keeps them that way); `samples` is ignored.

    drop: a blacklist, one value per bin of the layout (blacklist.readBlacklist).  A bin whose value is set leaves the mask
    as a bin that is empty in every sample does, and every later stage follows the mask (wc_newref_prep_gram_ex).
    ValueError for another length.
    """
    lib = _lib.load()
    ctx = _lib.context(device)
    if counts is None:
        chromBins = [max(len(s[str(c)]) for s in samples) for c in range(1, 23)]
        counts = samples_to_counts(samples, chromBins)
    else:
        chromBins = [int(v) for v in chrom_bins]
        counts = np.ascontiguousarray(counts, dtype=np.int32)
    n_s, n_total = counts.shape
    sizes = np.ascontiguousarray(chromBins, dtype=np.int64)
    mask = np.empty(n_total, dtype=np.uint8)
    mbins = np.empty(len(sizes), dtype=np.int64)
    n_b = ctypes.c_int64()
    on_gpu = _eig_on_gpu(n_s, pcacomp)
    gram = None if on_gpu else np.empty((n_s, n_s))
    if drop is not None:
        drop = np.ascontiguousarray(np.asarray(drop).reshape(-1) != 0, dtype=np.uint8)
        if len(drop) != n_total:
            raise ValueError('a blacklist of %d bins for a layout of %d' % (len(drop), n_total))
    _lib.check(lib.wc_newref_prep_gram_ex(ctx, _lib.ptr(counts), n_s, n_total, _lib.ptr(sizes), len(sizes),
                                          _lib.ptr(mask), _lib.ptr(mbins), ctypes.byref(n_b),
                                          None if on_gpu else _lib.ptr(gram), _lib.ptr(drop)))
    if on_gpu:          # the Gram matrix never leaves HBM
        evals, evecs = np.empty(pcacomp), np.empty((pcacomp, n_s))
        _lib.check(lib.wc_newref_prep_eig(ctx, int(pcacomp), _lib.ptr(evals), _lib.ptr(evecs)))
    else:
        evals, evecs = _leading_eigenpairs(gram, pcacomp)
    B = n_b.value
    comps = np.empty((pcacomp, B))
    mean = np.empty(B)
    if device_out:
        import torch
        dev = torch.device('cuda', device)
        masked = torch.empty((B, n_s), dtype=torch.float64, device=dev)
        corrected = torch.empty((B, n_s), dtype=torch.float64, device=dev)
        _lib.check(lib.wc_newref_prep_finish_dev(ctx, int(pcacomp), _lib.ptr(evecs), _lib.ptr(evals),
                                                 ctypes.c_void_p(masked.data_ptr()),
                                                 ctypes.c_void_p(corrected.data_ptr()), _lib.ptr(comps), _lib.ptr(mean)))
        return masked, chromBins, mask.astype(bool), corrected, comps, mean, [int(v) for v in mbins]
    masked = _pinned((B, n_s))
    corrected_t = _pinned((n_s, B))
    _lib.check(lib.wc_newref_prep_finish(ctx, int(pcacomp), _lib.ptr(evecs), _lib.ptr(evals), _lib.ptr(masked),
                                         _lib.ptr(corrected_t), _lib.ptr(comps), _lib.ptr(mean)))
    return masked, chromBins, mask.astype(bool), corrected_t.T, comps, mean, [int(v) for v in mbins]


# ---------------------------------------------------------------------------
# convert: BAM -> binned sample
# ---------------------------------------------------------------------------
CONVERT_KEYS = [str(c) for c in range(1, 23)] + ['X', 'Y']


class _Handle(object):
    """An object of the library in `_handle`, released once by the library function the subclass names in `_close`:
    close(), or leaving a `with` block."""
    _handle = None
    _close = None

    def close(self):
        if self._handle is not None:
            getattr(_lib.load(), self._close)(self._handle)
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _read_header(info_fn, refs_fn, handle, offsets=False):
    """The header of an opened reader: (info int64 [8], names, lengths) and, with `offsets`, the offsets [n_refs + 1].
    `info_fn` fills the info vector ([0] references, [5] bytes of their names), `refs_fn` the names with a newline
    between them, the lengths and the offsets."""
    info = np.zeros(8, dtype=np.int64)
    _lib.check(info_fn(handle, _lib.ptr(info)))
    n_refs, name_bytes = int(info[0]), int(info[5])
    names = ctypes.create_string_buffer(name_bytes + 1)
    tables = [np.zeros(n_refs, dtype=np.int64)] + ([np.zeros(n_refs + 1, dtype=np.int64)] if offsets else [])
    _lib.check(refs_fn(handle, ctypes.cast(names, ctypes.c_void_p), name_bytes + 1, *[_lib.ptr(t) for t in tables]))
    return [info, names.raw[:name_bytes].decode('latin1').split('\n')[:n_refs]] + tables


class BamReads(_Handle):
    """The placed records of a BAM file as the native reader (csrc/bamio.cpp) leaves them: `names`, `lengths`
    from the header, `offsets` [n_refs + 1] into `pos` (int32) / `mapq` (uint8) / `flag` (uint16) / `mate_pos` (int32,
    the next_pos field) -- views of the library's own memory, valid until close() -- and the record counts `mapped`,
    `unmapped`, `no_coordinate`."""
    _close = 'wc_bam_close'

    def __init__(self, path, threads=8):
        lib = _lib.load()
        handle = ctypes.c_void_p()
        _lib.check(lib.wc_bam_open(os.fsencode(path), int(threads), ctypes.byref(handle)))
        self._handle = handle
        info, self.names, self.lengths, self.offsets = _read_header(lib.wc_bam_info, lib.wc_bam_refs, handle, offsets=True)
        n_reads, self.mapped, self.unmapped, self.no_coordinate = (int(v) for v in info[1:5])
        if n_reads:
            self.pos = np.ctypeslib.as_array(ctypes.cast(lib.wc_bam_pos(handle), ctypes.POINTER(ctypes.c_int32)), (n_reads,))
            self.mapq = np.ctypeslib.as_array(ctypes.cast(lib.wc_bam_mapq(handle), ctypes.POINTER(ctypes.c_uint8)), (n_reads,))
            self.flag = np.ctypeslib.as_array(ctypes.cast(lib.wc_bam_flag(handle), ctypes.POINTER(ctypes.c_uint16)), (n_reads,))
            self.mate_pos = np.ctypeslib.as_array(ctypes.cast(lib.wc_bam_mate_pos(handle), ctypes.POINTER(ctypes.c_int32)),
                                                  (n_reads,))
        else:
            self.pos, self.mapq = np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8)
            self.flag, self.mate_pos = np.zeros(0, dtype=np.uint16), np.zeros(0, dtype=np.int32)

    def close(self):
        self.pos = self.mapq = self.flag = self.mate_pos = None      # the views go before the memory they look at
        _Handle.close(self)


class BamFile(_Handle):
    """The host stage of the device reader (csrc/bamfile.cpp, no GPU needed): the whole file in pinned host memory, its
    BGZF block directory, and the BAM header from as many leading blocks as it needs: `names`, `lengths`, `n_blocks`,
    `inflated_bytes` (the sum of ISIZE), `compressed_bytes`, `first_record` (offset of the first record in the inflated
    stream).  Errors carry the codes BamReads raises for the same file."""
    _close = 'wc_bamfile_close'

    def __init__(self, path, device=0):
        lib = _lib.load()
        handle = ctypes.c_void_p()
        _lib.check(lib.wc_bamfile_open(os.fsencode(path), int(device), ctypes.byref(handle)))
        self._handle = handle
        self.path = path
        info, self.names, self.lengths = _read_header(lib.wc_bamfile_info, lib.wc_bamfile_refs, handle)
        self.n_blocks, self.inflated_bytes, self.compressed_bytes, self.first_record = (int(v) for v in info[1:5])
        self.pinned = bool(info[6])
        self.pin_ms = float(info[7]) / 1e3          # of the pinned allocation, part of the open


class DeviceArray(object):
    """`n` elements of `dtype` at the device address `ptr`, owned by `reader` (a BamReadsDevice)."""

    def __init__(self, reader, ptr, n, dtype):
        self.reader, self.ptr, self.n, self.dtype = reader, ptr, n, np.dtype(dtype)

    def __len__(self):
        return self.n


#: device bytes BamReadsDevice may take for one file; 0: the library's rule (0.8 of the free device memory).  A file
#: that needs more takes the host reader (convertBam, convertbatch).
BAM_DEVICE_BUDGET = 0


class BamReadsDevice(_Handle):
    """BamReads with `pos` / `mapq` / `flag` / `mate_pos` born on the device (DeviceArray; csrc/bamgpu.hip: only the
    compressed bytes cross to the device, BGZF inflate and the record walk are kernels).  `source` is a path or an
    opened BamFile (which stays the caller's).  `budget`: device bytes the open may take (<= 0: BAM_DEVICE_BUDGET); a
    file that needs more raises with code E_LIMIT.  `stage_ms`: the open's stage times (wc_bam_dev_times)."""
    _close = 'wc_bam_dev_close'

    def __init__(self, source, device=0, budget=0):
        lib = _lib.load()
        own = not isinstance(source, BamFile)
        bamfile = BamFile(source, device=device) if own else source
        try:
            handle = ctypes.c_void_p()
            _lib.check(lib.wc_bam_open_dev(_lib.context(device), None, bamfile._handle,
                                           int(budget) if budget > 0 else int(BAM_DEVICE_BUDGET), ctypes.byref(handle)))
        finally:
            if own:
                bamfile.close()
        self._adopt(handle)

    def _adopt(self, handle):
        """The attributes of an opened wc_bam_dev handle."""
        lib = _lib.load()
        self._handle = handle
        info, self.names, self.lengths, self.offsets = _read_header(lib.wc_bam_dev_info, lib.wc_bam_dev_refs, handle,
                                                                    offsets=True)
        n_reads, self.mapped, self.unmapped, self.no_coordinate = (int(v) for v in info[1:5])
        self.device_bytes = int(info[6])
        self.n_reads = n_reads
        self.pos = DeviceArray(self, lib.wc_bam_dev_pos(handle), n_reads, np.int32)
        self.mapq = DeviceArray(self, lib.wc_bam_dev_mapq(handle), n_reads, np.uint8)
        self.flag = DeviceArray(self, lib.wc_bam_dev_flag(handle), n_reads, np.uint16)
        self.mate_pos = DeviceArray(self, lib.wc_bam_dev_mate_pos(handle), n_reads, np.int32)
        times = np.zeros(8, dtype=np.float64)
        _lib.check(lib.wc_bam_dev_times(handle, _lib.ptr(times)))
        self.stage_ms = dict(zip(('h2d', 'inflate', 'record_starts', 'link', 'checks', 'fields', 'order', 'call'),
                                 (float(v) for v in times)))

    def to_numpy(self):
        """(pos, mapq, flag, mate_pos) copied to host arrays."""
        out = (np.zeros(self.n_reads, dtype=np.int32), np.zeros(self.n_reads, dtype=np.uint8),
               np.zeros(self.n_reads, dtype=np.uint16), np.zeros(self.n_reads, dtype=np.int32))
        _lib.check(_lib.load().wc_bam_dev_fetch(self._handle, *[_lib.ptr(a) for a in out]))
        return out

    def close(self):
        self.pos = self.mapq = self.flag = self.mate_pos = None      # the views go before the memory they look at
        _Handle.close(self)


#: compressed bytes per chunk of BamReadsStream; 0: the library's default (wc_bam_stream_default_chunk)
BAM_STREAM_CHUNK = 0

STREAM_INFO_KEYS = ('chunks', 'largest_chunk_compressed_bytes', 'largest_chunk_inflated_bytes', 'largest_carry_bytes',
                    'peak_device_working_bytes', 'host_staging_bytes', 'output_regrows', 'pinned')


class BamReadsStream(BamReadsDevice):
    """BamReadsDevice by the streamed reader (wc_bam_stream_dev): the file goes through the GPU in chunks of whole BGZF
    blocks of at most `chunk` compressed bytes (<= 0: BAM_STREAM_CHUNK), records that straddle a chunk boundary are carried
    over, and host and device working memory are bounded by the chunk and the longest record.  The same attributes;
    `device_bytes` is the peak of the device memory, the four arrays included; `stage_ms` has 'reader_wait' (the call
    waiting for the file), 'device_wait' and 'call'; `stream_info` is wc_bam_dev_stream_info as a dict."""

    def __init__(self, path, device=0, chunk=0):
        lib = _lib.load()
        handle = ctypes.c_void_p()
        _lib.check(lib.wc_bam_stream_dev(_lib.context(device), None, os.fsencode(path),
                                         int(chunk) if chunk > 0 else int(BAM_STREAM_CHUNK), ctypes.byref(handle)))
        self._adopt(handle)
        times = np.zeros(8, dtype=np.float64)           # wc_bam_dev_times of a streamed handle: [0], [1] and [7] are set
        _lib.check(lib.wc_bam_dev_times(handle, _lib.ptr(times)))
        self.stage_ms = {'reader_wait': float(times[0]), 'device_wait': float(times[1]), 'call': float(times[7])}
        info = np.zeros(8, dtype=np.int64)
        _lib.check(lib.wc_bam_dev_stream_info(handle, _lib.ptr(info)))
        self.stream_info = dict(zip(STREAM_INFO_KEYS, (int(v) for v in info)))


class BamChunks(_Handle):
    """The host stage of the streamed reader (csrc/bamfile.cpp, no GPU needed): the header (`names`, `lengths`,
    `first_record`), then iteration over the chunks as dicts (first_block, blocks, compressed_bytes, inflated_bytes,
    file_offset, last).  Errors carry the codes of BamFile; a defect of a block is raised when its chunk is reached."""
    _close = 'wc_bamchunks_close'

    def __init__(self, path, device=0, chunk=0):
        lib = _lib.load()
        handle = ctypes.c_void_p()
        _lib.check(lib.wc_bamchunks_open(os.fsencode(path), int(device), int(chunk), ctypes.byref(handle)))
        self._handle = handle
        info, self.names, self.lengths = _read_header(lib.wc_bamchunks_info, lib.wc_bamchunks_refs, handle)
        self.compressed_bytes, self.first_record = int(info[3]), int(info[4])
        self.pinned, self.host_bytes = bool(info[6]), int(info[7])

    def __iter__(self):
        return self

    def __next__(self):
        out = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.load().wc_bamchunks_next(self._handle, _lib.ptr(out)))
        if not out[0]:
            raise StopIteration
        return {'first_block': int(out[1]), 'blocks': int(out[2]), 'compressed_bytes': int(out[3]),
                'inflated_bytes': int(out[4]), 'file_offset': int(out[5]), 'last': bool(out[6])}


#: the reader convertBam and convertbatch open a file with: 'device' (BamReadsDevice; the host reader only for a file
#: beyond the device budget), 'stream' (BamReadsStream: memory bounded by BAM_STREAM_CHUNK, no budget) or 'host' (BamReads);
#: 'bounded': no reader object at all, convertBam goes through convertBamBounded (openBamReads then opens the streamed reader).
#: Set by the measurement in profiles/convert_times.json:
#: 5 million records, whole call 0.285 s through the device reader against 0.517 s (spread 0.024 s) through the host reader.
CONVERT_READER = 'device'


def openBamReads(source, threads=8, device=0, stream=None, chunk=0):
    """The reader convertBam uses for `source` (a path or an opened BamFile).  With `stream` true, or None and
    CONVERT_READER == 'stream': the streamed device reader with chunks of `chunk` bytes (<= 0: BAM_STREAM_CHUNK).  Else with
    CONVERT_READER == 'device': the device reader, and the host reader where the file does not fit the device budget
    (E_LIMIT) -- the file's size decides, no option.  With 'host': the host reader."""
    if stream or (stream is None and CONVERT_READER in ('stream', 'bounded')):
        return BamReadsStream(source.path if isinstance(source, BamFile) else source, device=device, chunk=chunk)
    if CONVERT_READER == 'device':
        try:
            return BamReadsDevice(source, device=device)
        except _lib.WisecondorHipError as exc:
            if getattr(exc, 'code', None) != _lib.E_LIMIT:
                raise
    return BamReads(source.path if isinstance(source, BamFile) else source, threads=threads)


def convert_chromosome_key(name):
    """The sample-dict key of a BAM reference name (a leading 'chr' in any case dropped), None if it is skipped."""
    key = name[3:] if name[:3].lower() == 'chr' else name
    return key if key in CONVERT_KEYS else None


class _ConvertPlan(object):
    """What `convert` makes of the references `names` / `lengths` (header order) at `binsize`: `picked`, the (header
    index, sample key) of every processed chromosome; `refs`, those indices (int32); `n_bins` of each and `bin_offsets`
    [len(picked) + 1] into the flat counts of a call."""

    def __init__(self, names, lengths, binsize):
        picked = [(r, convert_chromosome_key(name)) for r, name in enumerate(names)]
        self.picked = [(r, key) for r, key in picked if key is not None]
        self.refs = np.asarray([r for r, _ in self.picked], dtype=np.int32)
        self.n_bins = [int(int(lengths[r]) / float(binsize) + 1) for r in self.refs]
        self.bin_offsets = np.concatenate([[0], np.cumsum(self.n_bins)]).astype(np.int64)
        self._listing = [(names[r], int(lengths[r])) for r in self.refs]

    def describe(self):
        """convertBam's line per processed chromosome"""
        for (name, length), bins in zip(self._listing, self.n_bins):
            print(name, 'length:', length, 'bins:', bins)

    def new_counts(self):
        return np.zeros(int(self.bin_offsets[-1]), dtype=np.int32)

    def sample(self, counts):
        """The sample dict of a call's flat counts (copies); a chromosome that is not in the header stays None."""
        chromosomes = dict((key, None) for key in CONVERT_KEYS)
        for i, (_, key) in enumerate(self.picked):
            chromosomes[key] = counts[self.bin_offsets[i]:self.bin_offsets[i + 1]].copy()
        return chromosomes

    @staticmethod
    def counters(stats):
        """The four filter counters and pair_fail out of a call's stats."""
        return {'filter_rmdup': int(stats[0]), 'filter_mapq': int(stats[1]), 'pre_retro': int(stats[2]),
                'post_retro': int(stats[3]), 'pair_fail': int(stats[6])}

    def spans(self, offsets):
        """[lo, hi) of every processed chromosome in arrays that reference r owns [offsets[r], offsets[r+1]) of; then the
        table of the same reads set side by side."""
        spans = [(int(offsets[r]), int(offsets[r + 1])) for r in self.refs]
        return spans, np.concatenate([[0], np.cumsum([hi - lo for lo, hi in spans])]).astype(np.int64)

    @staticmethod
    def contiguous(spans):
        return all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))

    @staticmethod
    def gather(array, spans, dtype):
        """The spans of a host array side by side, C-contiguous: a slice without a copy in the usual header order."""
        a = np.asarray(array)
        a = a[spans[0][0]:spans[-1][1]] if _ConvertPlan.contiguous(spans) else np.concatenate([a[lo:hi] for lo, hi in spans])
        return np.ascontiguousarray(a, dtype=dtype)


def convertReads(names, lengths, offsets, pos, mapq, binsize=1000000, minShift=4, threshold=4, device=0, verbose=False,
                 flag=None, mate_pos=None, minMapq=1, demandPair=False):
    """convertBam's filters and binning (wisetools.py:143-206) on reads that are already in arrays: references
    `names` / `lengths` in header order, reference r owning pos / mapq [offsets[r], offsets[r+1]).  One GPU call
    for all chromosomes (wc_convert_reads_ex).  `minMapq` is convertBam's `mapq` (the name is taken by the array);
    `demandPair` needs `flag` (uint16 flag words) and `mate_pos` parallel to `pos`.  The arrays are numpy arrays, or the
    DeviceArrays of a BamReadsDevice: those stay on the device (wc_convert_bam_dev hands their pointers to
    wc_convert_reads_ex_dev and gathers there where the picked references are not contiguous).  Returns (chromosomes
    dict, the four filter counters + pair_fail)."""
    lib = _lib.load()
    demandPair = bool(demandPair)
    if demandPair and (flag is None or mate_pos is None):
        raise ValueError('convertReads: demandPair needs the flag and mate_pos arrays')
    plan = _ConvertPlan(names, lengths, binsize)
    counts, stats = plan.new_counts(), np.zeros(8, dtype=np.int64)
    if plan.picked:
        if verbose:
            plan.describe()
        params = (float(binsize), int(minShift), int(threshold), int(minMapq), int(demandPair), _lib.ptr(plan.bin_offsets),
                  _lib.ptr(counts), _lib.ptr(stats))
        if isinstance(pos, DeviceArray):
            # the call works on the reader's own arrays and offsets: anything else would be silently ignored
            reader = pos.reader
            if not (isinstance(mapq, DeviceArray) and mapq.reader is reader and pos is reader.pos and mapq is reader.mapq):
                raise ValueError('convertReads: device arrays must be the pos / mapq of one BamReadsDevice')
            if demandPair and not (flag is reader.flag and mate_pos is reader.mate_pos):
                raise ValueError('convertReads: device flag / mate_pos must belong to the same BamReadsDevice')
            if not np.array_equal(np.asarray(offsets, dtype=np.int64), reader.offsets):
                raise ValueError('convertReads: with device arrays `offsets` must be the reader\'s own')
            _lib.check(lib.wc_convert_bam_dev(_lib.context(device), None, reader._handle, _lib.ptr(plan.refs), len(plan.picked),
                                              *params))
        else:
            spans, read_offsets = plan.spans(offsets)
            p, q = plan.gather(pos, spans, np.int32), plan.gather(mapq, spans, np.uint8)
            f = plan.gather(flag, spans, np.uint16) if demandPair else None
            m = plan.gather(mate_pos, spans, np.int32) if demandPair else None
            _lib.check(lib.wc_convert_reads_ex(_lib.context(device), _lib.ptr(p), _lib.ptr(q), _lib.ptr(f), _lib.ptr(m),
                                               _lib.ptr(read_offsets), len(plan.picked), *params))
    return plan.sample(counts), plan.counters(stats)


class ConvertRun(_Handle):
    """convertReads in resumable form (wc_convert_begin / feed / finish): the reads of the references `names` /
    `lengths` (header order) arrive in slices, in file order; every slice is filtered and binned as it arrives and only
    a small carry stays on the device, so the working memory follows the largest slice, not the read count.
    `feed(offsets, pos, mapq, flag, mate_pos)`: reference r owns [offsets[r], offsets[r+1]) of this slice's numpy arrays
    (references that are not processed are skipped); with `device_arrays` true the four are device addresses (ints)
    and the call returns as soon as the slice's kernels are enqueued on `stream`.  `finish()` returns what
    convertReads returns for the concatenation of the slices."""
    _close = 'wc_convert_end'

    def __init__(self, names, lengths, binsize=1000000, minShift=4, threshold=4, device=0, minMapq=1, demandPair=False):
        lib = _lib.load()
        self.demandPair = bool(demandPair)
        self.plan = _ConvertPlan(names, lengths, binsize)
        self.picked, self.bin_offsets = self.plan.picked, self.plan.bin_offsets
        if not self.picked:
            raise ValueError('ConvertRun: none of the references is a processed chromosome')
        handle = ctypes.c_void_p()
        _lib.check(lib.wc_convert_begin(_lib.context(device), len(self.picked), float(binsize), int(minShift), int(threshold),
                                        int(minMapq), int(self.demandPair), _lib.ptr(self.bin_offsets), ctypes.byref(handle)))
        self._handle = handle

    def feed(self, offsets, pos, mapq, flag=None, mate_pos=None, device_arrays=False, stream=None):
        lib = _lib.load()
        if self.demandPair and (flag is None or mate_pos is None):
            raise ValueError('ConvertRun.feed: demandPair needs the flag and mate_pos arrays')
        spans, slice_offsets = self.plan.spans(offsets)
        if device_arrays:
            if not self.plan.contiguous(spans):
                raise ValueError('ConvertRun.feed: device arrays must hold the processed references side by side')
            lo = spans[0][0]
            args = [ctypes.c_void_p(int(pos) + 4 * lo), ctypes.c_void_p(int(mapq) + lo),
                    ctypes.c_void_p(int(flag) + 2 * lo) if self.demandPair else None,
                    ctypes.c_void_p(int(mate_pos) + 4 * lo) if self.demandPair else None]
            _lib.check(lib.wc_convert_feed_dev(self._handle, ctypes.c_void_p(stream) if stream else None, *args,
                                               _lib.ptr(slice_offsets)))
            return
        p, q = self.plan.gather(pos, spans, np.int32), self.plan.gather(mapq, spans, np.uint8)
        f = self.plan.gather(flag, spans, np.uint16) if self.demandPair else None
        m = self.plan.gather(mate_pos, spans, np.int32) if self.demandPair else None
        _lib.check(lib.wc_convert_feed(self._handle, _lib.ptr(p), _lib.ptr(q), _lib.ptr(f), _lib.ptr(m),
                                       _lib.ptr(slice_offsets)))

    def info(self):
        """wc_convert_run_info: slices that ran, device bytes held, the bound of the carried positions."""
        out = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.load().wc_convert_run_info(self._handle, _lib.ptr(out)))
        return {'slices': int(out[0]), 'device_bytes': int(out[1]), 'carry_bound': int(out[2])}

    def finish(self):
        counts, stats = self.plan.new_counts(), np.zeros(8, dtype=np.int64)
        _lib.check(_lib.load().wc_convert_finish(self._handle, _lib.ptr(counts), _lib.ptr(stats)))
        return self.plan.sample(counts), self.plan.counters(stats)


def convertBamReads(bam, binsize=1000000, minShift=4, threshold=4, device=0, verbose=False, mapq=1, demandPair=False):
    """convertBam on an opened BamReads or BamReadsDevice: (chromosomes, qual_info)."""
    chromosomes, counters = convertReads(bam.names, bam.lengths, bam.offsets, bam.pos, bam.mapq, binsize, minShift,
                                         threshold, device=device, verbose=verbose, flag=bam.flag, mate_pos=bam.mate_pos,
                                         minMapq=mapq, demandPair=demandPair)
    qual_info = {'mapped': bam.mapped, 'unmapped': bam.unmapped, 'no_coordinate': bam.no_coordinate}
    qual_info.update(counters)
    return chromosomes, qual_info


BOUNDED_INFO_KEYS = ('chunks', 'largest_chunk_compressed_bytes', 'largest_carry_bytes', 'largest_carry_positions',
                     'peak_device_bytes', 'host_staging_bytes', 'placed_records', 'largest_chunk_inflated_bytes')


def convertBamBounded(bamfile, binsize=1000000, minShift=4, threshold=4, device=0, mapq=1, demandPair=False, chunk=0,
                      verbose=False, info=None):
    """convertBam by the bounded route (wc_convert_bam_stream_dev): the file goes through the GPU in chunks of at most
    `chunk` compressed bytes (<= 0: BAM_STREAM_CHUNK) as BamReadsStream reads it, and every chunk's reads are filtered
    and binned at once (ConvertRun's kernels) and dropped: device memory does not grow with the read count and the
    number of reads is not limited.  The same (chromosomes, qual_info).  `info`: a dict that receives BOUNDED_INFO_KEYS."""
    lib = _lib.load()
    with BamChunks(bamfile, device=-1, chunk=65536) as header:      # the header alone (host stage, ordinary memory)
        plan = _ConvertPlan(header.names, header.lengths, binsize)
    if not plan.picked:
        # nothing to bin: the reader alone gives the record counts (and the file's errors)
        with BamReadsStream(bamfile, device=device, chunk=chunk) as bam:
            return convertBamReads(bam, binsize, minShift, threshold, device=device, mapq=mapq, demandPair=demandPair)
    if verbose:
        plan.describe()
    counts, stats = plan.new_counts(), np.zeros(8, dtype=np.int64)
    out = np.zeros(16, dtype=np.int64)
    _lib.check(lib.wc_convert_bam_stream_dev(_lib.context(device), None, os.fsencode(bamfile),
                                             int(chunk) if chunk > 0 else int(BAM_STREAM_CHUNK), _lib.ptr(plan.refs),
                                             len(plan.picked), float(binsize), int(minShift), int(threshold), int(mapq),
                                             int(bool(demandPair)), _lib.ptr(plan.bin_offsets), _lib.ptr(counts),
                                             _lib.ptr(stats), _lib.ptr(out)))
    if info is not None:
        info.update(zip(BOUNDED_INFO_KEYS, (int(v) for v in out[:8])))
    qual_info = {'mapped': int(out[8]), 'unmapped': int(out[9]), 'no_coordinate': int(out[10])}
    qual_info.update(plan.counters(stats))
    return plan.sample(counts), qual_info


def convertBam(bamfile, binsize=1000000, minShift=4, threshold=4, threads=8, device=0, mapq=1, demandPair=False):
    """BAM file -> (dict chromosome -> int32[bins] or None, quality dict), wisetools.py:116-217: `mapq` the
    mapping-quality floor, `demandPair` the paired-end branch (only proper-pair first-in-pair reads take part, a
    duplicate has the previous such read's position and mate position, the rest is counted in pair_fail).  The file
    is read by the device reader (BamReadsDevice; the host reader BamReads with `threads` threads where the file does
    not fit the device budget; the streamed reader where CONVERT_READER says so: openBamReads), the filters run on the
    GPU.  With CONVERT_READER == 'bounded': convertBamBounded (chunks of BAM_STREAM_CHUNK bytes), no reader object."""
    if CONVERT_READER == 'bounded':
        return convertBamBounded(bamfile, binsize, minShift, threshold, device=device, mapq=mapq, demandPair=demandPair,
                                 verbose=True)
    with openBamReads(bamfile, threads=threads, device=device) as bam:
        return convertBamReads(bam, binsize, minShift, threshold, device=device, verbose=True, mapq=mapq,
                               demandPair=demandPair)


# ------------------------------------------------------- result files: deflate on the GPU ----
def deflateBound(row_bytes):
    """Most bytes one row of `row_bytes` bytes takes as a stream of deflateRows (wc_deflate_bound)."""
    return int(_lib.load().wc_deflate_bound(int(row_bytes)))


def deflateRows(rows, device=0, ctx=None, out_stride=None):
    """Every row of `rows` as one raw deflate stream (zlib.decompress(x, -15) reads it) and its CRC-32, made on the
    GPU (wc_deflate_rows: run-length matches and a Huffman code per block of wc_deflate_block_bytes() bytes).
    rows: 2-d, a numpy array (any dtype; the rows' bytes in memory order, rows may be strided) or a torch tensor on the
    GPU.  Returns (streams uint8 [n, out_stride], lengths int64 [n], crcs uint32 [n]) of the same kind: numpy arrays, or
    tensors that stay on the device (crcs then int32: the same 32 bits).  Row i is streams[i, :lengths[i]]; the bytes
    behind it mean nothing.  out_stride defaults to deflateBound(bytes per row)."""
    lib = _lib.load()
    if isinstance(rows, np.ndarray):
        assert rows.ndim == 2 and (rows.shape[1] == 0 or rows.strides[1] == rows.itemsize) and rows.strides[0] >= 0
        n, row_bytes = rows.shape[0], rows.shape[1] * rows.itemsize
        src_stride = rows.strides[0] if n > 1 else row_bytes
        assert src_stride >= row_bytes
        stride = int(out_stride or deflateBound(row_bytes))
        streams = np.zeros((n, stride), dtype=np.uint8)
        lengths = np.zeros(n, dtype=np.int64)
        crcs = np.zeros(n, dtype=np.uint32)
        if n:
            _lib.check(lib.wc_deflate_rows(ctx or _lib.context(device), ctypes.c_void_p(rows.ctypes.data), n, row_bytes,
                                           src_stride, _lib.ptr(streams), stride, _lib.ptr(lengths), _lib.ptr(crcs)))
        return streams, lengths, crcs
    import torch
    assert rows.is_cuda and rows.dim() == 2 and (rows.shape[1] == 0 or rows.stride(1) == 1)
    item = rows.element_size()
    n, row_bytes = int(rows.shape[0]), int(rows.shape[1]) * item
    src_stride = int(rows.stride(0)) * item if n > 1 else row_bytes
    assert src_stride >= row_bytes
    stride = int(out_stride or deflateBound(row_bytes))
    dev = rows.device
    streams = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    lengths = torch.empty((n,), dtype=torch.int64, device=dev)
    crcs = torch.empty((n,), dtype=torch.int32, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.check(lib.wc_deflate_rows_dev(ctx or _lib.context(dev.index or 0), torch.cuda.current_stream().cuda_stream,
                                               rows.data_ptr(), n, row_bytes, src_stride, streams.data_ptr(), stride,
                                               lengths.data_ptr(), crcs.data_ptr()))
    return streams, lengths, crcs


class ResultMembers(object):
    """The framing of the members results_r.npy / results_z.npy for one set of chromosome sizes, on the device: the
    member with gaps for the values (wc_results_member_template), uploaded once.  image(rows) writes the members of a
    batch of dense float64 rows [n, sum(chrom_sizes)] that live on the device (wc_results_members_dev)."""

    def __init__(self, chrom_sizes, device):
        import torch
        lib = _lib.load()
        sizes = np.ascontiguousarray(chrom_sizes, dtype=np.int64)
        self.n_total = int(sizes.sum())
        self.n_gaps = len(sizes)
        self.member_bytes = int(lib.wc_results_member_bytes(_lib.ptr(sizes), len(sizes)))
        if self.member_bytes < 0 or self.n_gaps > 64:
            raise ValueError('result members: unusable chromosome sizes')
        tmpl = np.zeros(self.member_bytes, dtype=np.uint8)
        table = np.zeros(3 * len(sizes), dtype=np.int64)
        _lib.check(lib.wc_results_member_template(_lib.ptr(sizes), len(sizes), _lib.ptr(tmpl), len(tmpl), _lib.ptr(table)))
        self.device = torch.device(device)
        self.template = torch.from_numpy(tmpl).to(self.device)
        self.table = torch.from_numpy(table).to(self.device)
        self.stride = (self.member_bytes + 15) // 16 * 16

    def image(self, rows, ctx=None):
        """uint8 tensor [n, member_bytes] (rows `stride` bytes apart): the member of every row of `rows`."""
        import torch
        assert rows.is_cuda and rows.dtype == torch.float64 and rows.dim() == 2 and rows.shape[1] == self.n_total
        assert rows.shape[1] == 0 or rows.stride(1) == 1
        n = int(rows.shape[0])
        out = torch.empty((n, self.stride), dtype=torch.uint8, device=rows.device)
        done = 0
        while done < n:                                 # (the kernel's grid takes 65 535 rows)
            part = min(n - done, 65535)
            with torch.cuda.device(rows.device):
                _lib.check(_lib.load().wc_results_members_dev(
                    ctx or _lib.context(rows.device.index or 0), torch.cuda.current_stream().cuda_stream,
                    self.template.data_ptr(), self.member_bytes, self.table.data_ptr(), self.n_gaps, rows[done:].data_ptr(),
                    int(rows.stride(0)) if n > 1 else self.n_total, part, out[done:].data_ptr(), self.stride))
            done += part
        return out[:, :self.member_bytes]


# ------------------------------------------------------------------- plotbatch: z-score panel PNGs ----
def loadCytoBands(cytoFile):
    """chromosome name -> [(start, end, stain)] of a UCSC cytoBand table, read once.  Upstream's loadCytoBands
    (wisetools.py:73-86) never stores the table's last chromosome and plotLines then dies on it; here every
    chromosome of the table is kept and one that is absent simply has no bands."""
    table = {}
    with open(cytoFile, 'r') as cytoData:
        for line in cytoData:
            parts = line.split()
            if parts:
                table.setdefault(parts[0][3:], []).append((parts[1], parts[2], parts[4]))
    return table


def plotBands(table, chromosomes, binsize):
    """The bands of the plotted chromosomes in bins (wisetools.py:566-598): float64 [n, 4] rows (x0, x1, alpha, hatch:
    0 none, 1 '//', 2 '\\', -1 no rectangle) and the offsets int32 [panels + 1] of every panel's rows.  gneg and other
    stains get no rectangle but keep their row: the reference draws the -1.5 thr line once per band of the table,
    whatever its stain, so a panel has that line exactly when it has rows here."""
    rows, offs = [], [0]
    for chrom in chromosomes:
        for start, end, stain in table.get(str(chrom), []):
            x0, x1 = float(start) / binsize, float(end) / binsize
            if stain[1:4] == 'pos':
                rows.append((x0, x1, float(stain[4:]) / 100 * 0.5, 0.0))
            elif stain == 'acen':
                rows.append((x0, x1, 1 * 0.5, 1.0))
            elif stain == 'gvar':
                rows.append((x0, x1, 0.75 * 0.5, 2.0))
            else:
                rows.append((x0, x1, 0.0, -1.0))
        offs.append(len(rows))
    return np.array(rows, dtype=np.float64).reshape(-1, 4), np.array(offs, dtype=np.int32)


def plotImageSize(size, dpi):
    """(width, height) in pixels of a figure of size[0] x size[1] inches."""
    return int(np.floor(size[0] * dpi + 0.5)), int(np.floor(size[1] * dpi + 0.5))


def plotLayout(width, height, rows, columns, n_panels):
    """The panels' pixel boxes [x0, y0, x1, y1), int32 [n_panels, 4] (wc_plot_layout; host only)."""
    boxes = np.zeros((n_panels, 4), dtype=np.int32)
    _lib.check(_lib.load().wc_plot_layout(int(width), int(height), int(rows), int(columns), int(n_panels), _lib.ptr(boxes)))
    return boxes


def _dense_rows(arrays_list, sizes, out=None):
    """Per-sample lists of per-chromosome arrays of the lengths `sizes` -> float64 rows [n, max(sum(sizes), 1)], every
    sample's arrays end to end (written into `out` where one is given)."""
    total = int(np.sum(sizes))
    rows = np.zeros((len(arrays_list), max(total, 1)), dtype=np.float64) if out is None else out
    for i, arrays in enumerate(arrays_list):
        if [len(c) for c in arrays] != [int(v) for v in sizes]:
            raise ValueError('sample %d has other chromosome lengths than the first' % i)
        if total:
            rows[i, :total] = np.concatenate([np.asarray(c, dtype=np.float64) for c in arrays])
    return rows


def _dense_results(zs_list, calls_list, max_calls=None):
    """Per-sample lists of per-chromosome z arrays and call tables -> the dense layout wc_test_batch_dev leaves on the
    device: rows [n, total], sizes int64 [n_chrom], calls [n, max_calls, 5], n_calls int32 [n]."""
    sizes = np.array([len(c) for c in zs_list[0]], dtype=np.int64)
    rows = _dense_rows(zs_list, sizes)
    tables = [np.asarray(c, dtype=np.float64).reshape(-1, 5) for c in calls_list]      # (an empty list is stored with shape (0,))
    cap = max([len(t) for t in tables] + [1]) if max_calls is None else int(max_calls)
    calls = np.zeros((len(tables), cap, 5), dtype=np.float64)
    n_calls = np.zeros(len(tables), dtype=np.int32)
    for i, t in enumerate(tables):
        calls[i, :len(t)] = t
        n_calls[i] = len(t)
    return rows, sizes, calls, n_calls


def plotList(zs_list, calls_list, threshold, chromosomes=range(1, 23), mineffect=0, capacity=None, device=0):
    """The display lists the GPU makes of the samples' z-scores and calls (wc_plot_list): entries float64 [n, panels,
    capacity, 9] rows (kind, panel, x0, x1, y0, y1, colour id, alpha, value), counts int32 [n, panels] of the entries
    every panel needs, and the status word (bit 0: some panel needs more than `capacity`; default: the worst case)."""
    rows, sizes, calls, n_calls = _dense_results(zs_list, calls_list)
    panels = np.array(list(chromosomes), dtype=np.int32)
    if capacity is None:
        capacity = 1 + (int(max([sizes[c - 1] for c in panels] + [0])) + 1) // 2 + calls.shape[1]
    n = rows.shape[0]
    entries = np.zeros((n, len(panels), int(capacity), 9), dtype=np.float64)
    counts = np.zeros((n, len(panels)), dtype=np.int32)
    status = np.zeros(1, dtype=np.int32)
    _lib.check(_lib.load().wc_plot_list(_lib.context(device), _lib.ptr(rows), rows.shape[1], n, _lib.ptr(sizes), len(sizes),
                                        _lib.ptr(calls), _lib.ptr(n_calls), calls.shape[1], float(threshold), float(mineffect),
                                        _lib.ptr(panels), len(panels), int(capacity), _lib.ptr(entries), _lib.ptr(counts),
                                        _lib.ptr(status)))
    return entries, counts, int(status[0])


def _assemble(stream, bytes_of, assemble):
    """The file one of the library's assemblers puts around a raw deflate stream: bytes_of(stream length) sizes the room,
    assemble(stream, its length, room, its size, where the file's length goes) fills it."""
    stream = np.ascontiguousarray(np.frombuffer(bytes(stream), dtype=np.uint8))
    out = np.zeros(max(1, int(bytes_of(len(stream)))), dtype=np.uint8)
    n = np.zeros(1, dtype=np.int64)
    _lib.check(assemble(_lib.ptr(stream), len(stream), _lib.ptr(out), len(out), _lib.ptr(n)))
    return out[:int(n[0])].tobytes()


def pngAssemble(width, height, stream, adler):
    """The PNG file of one image from its raw deflate stream and the Adler-32 of its scanlines (wc_png_assemble; host
    only): signature, IHDR, IDAT = 78 01 + stream + Adler-32, IEND."""
    lib = _lib.load()
    return _assemble(stream, lib.wc_png_bytes, lambda s, n, *room: lib.wc_png_assemble(int(width), int(height), s, n,
                                                                                      int(adler) & 0xffffffff, *room))


def adler32Rows(rows, device=0):
    """zlib.adler32 of every row of a 2-d uint8 array, computed on the GPU (wc_adler32_rows_dev)."""
    import torch
    rows = np.ascontiguousarray(rows, dtype=np.uint8)
    assert rows.ndim == 2
    n, row_bytes = rows.shape
    dev = torch.device('cuda', device)
    out = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev)
    src = torch.from_numpy(rows).to(dev) if rows.size else torch.zeros((1,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().wc_adler32_rows_dev(_lib.context(device), torch.cuda.current_stream().cuda_stream, src.data_ptr(), n,
                                                   row_bytes, row_bytes, out.data_ptr()))
        torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)[:n]


def sampleNameOf(infile):
    """The sample name of the title, as upstream toolPlot takes it from the file name (wisecondor.py:286)."""
    return infile.split('/')[-1].split('.')[0]


def _plot_job(what, results, names, cytofile, chromosomes):
    """What plot_batch and plot_pdf_batch (`what`) make of their arguments before they differ: the dense rows, sizes, calls
    and n_calls of _dense_results, panels (int32), bands and band_off (plotBands; None without a cytofile), name_cap and
    the samples' thresholds, as attributes of one object.  None: there are no results."""
    import types
    if len(results) != len(names):
        raise ValueError('%s: %d results, %d names' % (what, len(results), len(names)))
    if not results:
        return None
    chromosomes = [int(c) for c in chromosomes]
    binsize = np.asarray(results[0]['binsize']).item()
    for i, res in enumerate(results):
        if np.asarray(res['binsize']).item() != binsize:
            raise ValueError('sample %d has another bin size than the first' % i)
    rows, sizes, calls, n_calls = _dense_results([list(res['results_z']) for res in results], [res['results_calls'] for res in results])
    bands = band_off = None
    if cytofile is not None:
        table = cytofile if isinstance(cytofile, dict) else loadCytoBands(cytofile)
        bands, band_off = plotBands(table, chromosomes, binsize)
    return types.SimpleNamespace(rows=rows, sizes=sizes, calls=calls, n_calls=n_calls, panels=np.array(chromosomes, dtype=np.int32),
                                 bands=bands, band_off=band_off,
                                 name_cap=max(len(n.encode('latin1', 'replace')) for n in names) + 1,
                                 thresholds=[float(np.asarray(res['threshold_z']).item()) for res in results])


def _threshold_groups(job, names):
    """Per threshold_z value of a _plot_job, ascending -- one GPU call each: (threshold, the samples' indices, their names
    as a zero-padded uint8 block [n, name_cap], their contiguous z rows, calls and call counts)."""
    for thr in sorted(set(job.thresholds)):
        pick = [i for i, t in enumerate(job.thresholds) if t == thr]
        name_block = np.zeros((len(pick), job.name_cap), dtype=np.uint8)
        for k, i in enumerate(pick):
            raw = names[i].encode('latin1', 'replace')
            name_block[k, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        yield (thr, pick, name_block, np.ascontiguousarray(job.rows[pick]), np.ascontiguousarray(job.calls[pick]),
               np.ascontiguousarray(job.n_calls[pick]))


def plot_batch(results, names, cytofile=None, chromosomes=range(1, 23), columns=2, size=(11.7, 8.3), mineffect=0, dpi=100,
               device=0, ctx=None, details=None):
    """The z-score panel plots of upstream `plot` (plotLines, wisetools.py:527-662) for a batch of `test` results, drawn,
    checksummed and deflated on the GPU (wc_plot_batch): a list of PNG files as bytes, one per result.
    results   per sample a mapping with results_z (per-chromosome arrays), results_calls, threshold_z and binsize, as a
              result file holds them; all must share their chromosome lengths and bin size
    names     the sample names of the titles
    cytofile  a cytoBand table (or an already loaded one: loadCytoBands), None: no bands
    details   a dict that receives 'scanlines' (uint8 [n, height, 1 + 3 width]; not when it holds want_scanlines =
              False), 'size' and 'times_ms' (per GPU call: copy in, list, raster, Adler-32, deflate, copy out), for tests
              and measurements
    Samples with different threshold_z values take one GPU call per value."""
    job = _plot_job('plot_batch', results, names, cytofile, chromosomes)
    if job is None:
        return []
    lib = _lib.load()
    sizes, panels, bands, band_off, name_cap = job.sizes, job.panels, job.bands, job.band_off, job.name_cap
    width, height = plotImageSize(size, dpi)
    image = int(lib.wc_plot_image_bytes(width, height))
    if image < 0:
        raise ValueError('plot_batch: %d x %d pixels' % (width, height))
    stride = int(lib.wc_deflate_bound(image))
    out = [None] * len(results)
    scan = np.zeros((len(results), image), dtype=np.uint8) if details is not None and details.get('want_scanlines', True) else None
    times = []
    handle = ctx or _lib.context(device)
    for thr, pick, name_block, z_part, c_part, k_part in _threshold_groups(job, names):
        n = len(pick)
        streams = np.zeros((n, stride), dtype=np.uint8)
        lengths = np.zeros(n, dtype=np.int64)
        adlers = np.zeros(n, dtype=np.uint32)
        lines = np.zeros((n, image), dtype=np.uint8) if scan is not None else None
        t_ms = np.zeros(8, dtype=np.float64) if details is not None else None
        _lib.check(lib.wc_plot_batch(handle, _lib.ptr(z_part), z_part.shape[1], n, _lib.ptr(sizes), len(sizes), _lib.ptr(c_part),
                                     _lib.ptr(k_part), c_part.shape[1], thr, float(mineffect), _lib.ptr(panels), len(panels),
                                     int(columns), _lib.ptr(bands), _lib.ptr(band_off), _lib.ptr(name_block), name_cap, width, height,
                                     int(dpi), _lib.ptr(lines), _lib.ptr(streams), stride, _lib.ptr(lengths), _lib.ptr(adlers),
                                     _lib.ptr(t_ms)))
        for k, i in enumerate(pick):
            out[i] = pngAssemble(width, height, streams[k, :lengths[k]], adlers[k])
            if scan is not None:
                scan[i] = lines[k]
        if t_ms is not None:
            times.append(t_ms[:6].tolist())
    if details is not None:
        if scan is not None:
            details['scanlines'] = scan.reshape(len(results), height, 1 + 3 * width)
        details['times_ms'] = times
        details['size'] = (width, height)
    return out


# ------------------------------------------------------------------- plotpdf: vector PDF pages ----
def pdfPageSize(size):
    """(width, height) of a page of size[0] x size[1] inches in centipoints (1 / 100 pt)."""
    return int(np.floor(size[0] * 7200 + 0.5)), int(np.floor(size[1] * 7200 + 0.5))


def pdfSections(sizes, chromosomes, band_off, slots, name_cap):
    """The section starts of a page's content for the given slot counts per panel, int64 [11 panels + 3], the last entry
    the row's bytes (wc_plot_pdf_sections; host only)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    panels = np.ascontiguousarray(list(chromosomes), dtype=np.int32)
    slots = np.ascontiguousarray(slots, dtype=np.int32)
    band_off = None if band_off is None else np.ascontiguousarray(band_off, dtype=np.int32)
    starts = np.zeros(11 * len(panels) + 3, dtype=np.int64)
    if len(slots) != len(panels) or _lib.load().wc_plot_pdf_sections(_lib.ptr(sizes), len(sizes), _lib.ptr(panels), len(panels),
                                                                  _lib.ptr(band_off), _lib.ptr(slots), int(name_cap),
                                                                  _lib.ptr(starts)) < 0:
        raise ValueError('pdfSections: unusable arguments')
    return starts


def pdfAssemble(width_cp, height_cp, stream, adler):
    """The PDF file of one page from the raw deflate stream of its content and the content's Adler-32 (wc_pdf_assemble;
    host only): header, Catalog, Pages, Page, the font Courier, the graphics states /A000 .. /A255, the two hatch patterns,
    the content object = 78 01 + stream + Adler-32, xref, trailer."""
    lib = _lib.load()
    return _assemble(stream, lib.wc_pdf_bytes, lambda s, n, *room: lib.wc_pdf_assemble(int(width_cp), int(height_cp), s, n,
                                                                                      int(adler) & 0xffffffff, *room))


def plot_pdf_batch(results, names, cytofile=None, chromosomes=range(1, 23), columns=2, size=(11.7, 8.3), mineffect=0, device=0,
                   ctx=None, details=None):
    """The z-score panel plots of upstream `plot` as vector PDF pages, the content streams written, checksummed and
    deflated on the GPU (wc_plot_pdf_batch): a list of PDF files as bytes, one per result.  Arguments as plot_batch's.
    details   a dict that receives 'content' (per sample the uncompressed content stream, bytes; not when it holds
              want_content = False), 'row_bytes' and 'offsets' (per GPU call: the bytes of every sample's stream and its
              section starts), 'size' (the page in centipoints) and 'times_ms' (per GPU call: copy in, list, content,
              Adler-32, deflate, copy out)
    Samples with different threshold_z values take one GPU call per value."""
    job = _plot_job('plot_pdf_batch', results, names, cytofile, chromosomes)
    if job is None:
        return []
    lib = _lib.load()
    sizes, panels, bands, band_off, name_cap = job.sizes, job.panels, job.bands, job.band_off, job.name_cap
    width, height = pdfPageSize(size)
    bound = int(lib.wc_plot_pdf_row_bound(_lib.ptr(sizes), len(sizes), _lib.ptr(panels), len(panels), _lib.ptr(band_off),
                                          job.calls.shape[1], name_cap))
    if bound < 0:
        raise ValueError('plot_pdf_batch: unusable chromosomes, cytoband table or names')
    stride = int(lib.wc_deflate_bound(bound))
    out = [None] * len(results)
    content = [None] * len(results)
    times, row_bytes, offsets = [], [], []
    handle = ctx or _lib.context(device)
    for thr, pick, name_block, z_part, c_part, k_part in _threshold_groups(job, names):
        n = len(pick)
        # (rows of the worst case's size: the pages they hold are written, the rest is never touched)
        streams = np.zeros((n, stride), dtype=np.uint8)
        lengths = np.zeros(n, dtype=np.int64)
        adlers = np.zeros(n, dtype=np.uint32)
        lines = np.zeros((n, bound), dtype=np.uint8) if details is not None and details.get('want_content', True) else None
        t_ms = np.zeros(8, dtype=np.float64) if details is not None else None
        used = np.zeros(1, dtype=np.int64)
        starts = np.zeros(11 * len(panels) + 3, dtype=np.int64)
        _lib.check(lib.wc_plot_pdf_batch(handle, _lib.ptr(z_part), z_part.shape[1], n, _lib.ptr(sizes), len(sizes), _lib.ptr(c_part),
                                         _lib.ptr(k_part), c_part.shape[1], thr, float(mineffect), _lib.ptr(panels), len(panels),
                                         int(columns), _lib.ptr(bands), _lib.ptr(band_off), _lib.ptr(name_block), name_cap, width,
                                         height, _lib.ptr(lines), bound, _lib.ptr(streams), stride, _lib.ptr(lengths),
                                         _lib.ptr(adlers), _lib.ptr(used), _lib.ptr(starts), _lib.ptr(t_ms)))
        for k, i in enumerate(pick):
            out[i] = pdfAssemble(width, height, streams[k, :lengths[k]], adlers[k])
            if lines is not None:
                content[i] = lines[k, :int(used[0])].tobytes()
        if t_ms is not None:
            times.append(t_ms[:6].tolist())
        row_bytes.append(int(used[0]))
        offsets.append(starts)
    if details is not None:
        details['content'] = content
        details['row_bytes'] = row_bytes
        details['offsets'] = offsets
        details['times_ms'] = times
        details['size'] = (width, height)
    return out


# ------------------------------------------------------------------- exportjson: lossless JSON ----
JSON_KEYS = ('binsize', 'threshold_z', 'asdef', 'aasdef', 'arguments', 'results_cwz', 'results_calls', 'results_z', 'results_r')


def formatDoubles(values, strict=False, device=None):
    """The text json.dumps gives for every float64 of `values`, as a list of bytes (wc_format_doubles_host; with a
    device number wc_format_doubles, the same routine in the GPU's kernel)."""
    lib = _lib.load()
    v = np.ascontiguousarray(values, dtype=np.float64).ravel()
    text = np.zeros((len(v), 24), dtype=np.uint8)
    lens = np.zeros(len(v), dtype=np.uint8)
    if device is None:
        _lib.check(lib.wc_format_doubles_host(_lib.ptr(v), len(v), int(bool(strict)), _lib.ptr(text), _lib.ptr(lens)))
    else:
        _lib.check(lib.wc_format_doubles(_lib.context(device), _lib.ptr(v), len(v), int(bool(strict)), _lib.ptr(text), _lib.ptr(lens)))
    flat = text.tobytes()
    return [flat[24 * i:24 * i + int(n)] for i, n in enumerate(lens)]


def jsonRowBound(sizes):
    """Most bytes the JSON text of one dense row takes (wc_json_row_bound; host only)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    bound = int(_lib.load().wc_json_row_bound(_lib.ptr(sizes), len(sizes)))
    if bound < 0:
        raise ValueError('jsonRowBound: unusable chromosome sizes')
    return bound


def jsonRows(rows, sizes, strict=False, device=0, ctx=None, row_stride=None, times=None):
    """The compact JSON text [[v,...],[...],...] of every dense float64 row (host array [n, >= sum(sizes)]), written on
    the GPU (wc_json_rows): a list of bytes.  times: a list that receives [copy in, lengths and scan, bytes, copy out] ms."""
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    n = rows.shape[0]
    stride = jsonRowBound(sizes)
    text = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int64)
    t_ms = np.zeros(4, dtype=np.float64) if times is not None else None
    _lib.check(lib.wc_json_rows(ctx or _lib.context(device), _lib.ptr(rows), int(rows.shape[1] if row_stride is None else row_stride), n,
                                _lib.ptr(sizes), len(sizes), int(bool(strict)), _lib.ptr(text), stride, _lib.ptr(lens), _lib.ptr(t_ms)))
    if times is not None:
        times.extend(t_ms.tolist())
    return [text[i, :lens[i]].tobytes() for i in range(n)]


def _text_export_batch(results, keys, sizes, bound, lead, room, min_len, text_call, pack, piece, device, ctx, max_rows, max_bytes,
                       details):
    """The GPU calls of export_json_batch and export_tracks_batch.  Per GPU call: the dense rows of results_<key> for every
    key of `keys` (all of the first key, then all of the second) through a pinned staging array, the text of every row
    `lead` bytes into its slot of lead + `room` bytes (text_call(handle, stream, rows, row_stride, n_rows, text,
    text_stride, text_len, second): pointers of device memory), the optional pack stage, ONE read-back of the rows'
    int64 counters [text_len, the text call's second counter, packed length] and the 32-bit CRCs, the range checks
    (text_len in min_len .. bound), and per-row copies of the used bytes alone.
    pack: None or (max_row_bytes, out_stride, least, call): call(handle, stream, text, counts, n, files) packs the rows
    of `text` [rows, stride] into `files` [rows, out_stride] and leaves counts[2] (at least `least`) and, where it has
    them, the rows' CRC-32 as the 32-bit words of counts[3]; n: results in this call.
    piece(data, k, text_len, crc): the output bytes of a row of keys[k] from the uint8 array copied for it.
    A batch is split at max_rows rows and at max_bytes of device memory per GPU call.  details (may be None) receives
    'times_ms': per GPU call [copy in, text, pack, copy out].
    Returns (pieces, text_bytes, second): per result a tuple over the keys."""
    import torch
    total = int(sizes.sum())
    stride = lead + max(16, (room + 15) // 16 * 16)
    max_row_bytes, out_stride, least, pack_call = pack or (0, 0, 0, None)
    # device bytes of a row: the values, their digits between the passes, the text; packed: the blocks' slots and the file
    per_row = 24 * max(total, 1) + stride + (2 * out_stride + 64 * (max_row_bytes // int(_lib.load().wc_deflate_block_bytes()) + 1) if pack else 0)
    per_call = max(1, min(int(max_rows), int(max_bytes) // per_row) // len(keys))
    dev = torch.device('cuda', device)
    handle = ctx or _lib.context(device)
    pieces, text_bytes, second, times = [], [], [], []
    for at in range(0, len(results), per_call):
        part = results[at:at + per_call]
        n, rows_n = len(part), len(part) * len(keys)
        rows = _pinned((rows_n, max(total, 1)))
        for k, key in enumerate(keys):
            _dense_rows([res['results_' + key] for res in part], sizes, out=rows[k * n:(k + 1) * n])
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(5)] if details is not None else None
            if marks:
                marks[0].record()
            d_rows = torch.from_numpy(rows).to(dev, non_blocking=True)
            text = torch.empty((rows_n, stride), dtype=torch.uint8, device=dev)
            counts = torch.empty((4, rows_n), dtype=torch.int64, device=dev)
            if marks:
                marks[1].record()
            text_call(handle, stream, d_rows.data_ptr(), rows.shape[1], rows_n, text.data_ptr() + lead, stride, counts[0].data_ptr(),
                      counts[1].data_ptr())
            if marks:
                marks[2].record()
            if pack:
                files = torch.empty((rows_n, out_stride), dtype=torch.uint8, device=dev)
                pack_call(handle, stream, text, counts, n, files)
            if marks:
                marks[3].record()
            h_counts = counts.cpu().numpy()
            h_crc = h_counts[3].view(np.uint32)
            if np.any(h_counts[0] < min_len) or np.any(h_counts[0] > bound):
                raise _lib.WisecondorHipError('a text row of %d bytes, the bound is %d' % (int(h_counts[0].max()), bound))
            if pack and (np.any(h_counts[2] < least) or np.any(h_counts[2] > out_stride)):
                raise _lib.WisecondorHipError('a packed row of %d bytes' % int(h_counts[2].max()))
            used, src = (h_counts[2], files) if pack else (h_counts[0], text[:, lead:])
            flat = [piece(src[i, :int(used[i])].cpu().numpy(), i // n, int(h_counts[0][i]), int(h_crc[i])) for i in range(rows_n)]
            if marks:
                marks[4].record()
                marks[4].synchronize()
                times.append([marks[k].elapsed_time(marks[k + 1]) for k in range(4)])
        for i in range(n):
            at_row = [k * n + i for k in range(len(keys))]
            pieces.append(tuple(flat[j] for j in at_row))
            text_bytes.append(tuple(int(h_counts[0][j]) for j in at_row))
            second.append(tuple(int(h_counts[1][j]) for j in at_row))
    if details is not None:
        details['times_ms'] = times
    return pieces, text_bytes, second


def gzipAssemble(stream, crc, input_len):
    """One gzip member around a raw deflate stream (wc_gzip_assemble; host only): a fixed header without name or time, the
    stream, the CRC-32 and the length of the uncompressed bytes."""
    lib = _lib.load()
    return _assemble(stream, lib.wc_gzip_bytes, lambda s, n, *room: lib.wc_gzip_assemble(s, n, int(crc) & 0xffffffff, int(input_len), *room))


def _json_plain(value):
    """(True, the value as json.dumps takes it) for bool, int, float, str, None and lists or tuples of those (numpy scalars
    through .item()); (False, None) for everything else."""
    if isinstance(value, np.generic):
        value = value.item()
    if value is None or isinstance(value, (bool, int, float, str)):
        return True, value
    if isinstance(value, (list, tuple)):
        items = [_json_plain(v) for v in value]
        if all(ok for ok, _ in items):
            return True, [v for _, v in items]
    return False, None


def jsonArguments(arguments):
    """The `arguments` of a result file as the export keeps them: the entries _json_plain takes, keys sorted; everything
    else (the `func` entry, nested objects) is left out."""
    kept = {}
    for key in sorted(arguments, key=str):
        ok, value = _json_plain(arguments[key])
        if ok:
            kept[str(key)] = value
    return kept


def _json_nulls(value):
    """`value` with every float that is not finite replaced by None."""
    if isinstance(value, float):
        return value if value - value == 0 else None
    if isinstance(value, list):
        return [_json_nulls(v) for v in value]
    if isinstance(value, dict):
        return {k: _json_nulls(v) for k, v in value.items()}
    return value


def jsonHead(result, strict=False):
    """The host's part of an exported file: '{' and the keys binsize .. results_calls (JSON_KEYS), without the closing
    brace, as bytes.  result: a dict with binsize, threshold_z, asdef, aasdef (scalars, written as .item() gives them),
    arguments (a dict), results_cwz and results_calls (rows [int, int, int, float, float]; empty: [])."""
    import json
    calls = np.asarray(result['results_calls'], dtype=np.float64).reshape(-1, 5)
    head = {key: np.asarray(result[key]).item() for key in JSON_KEYS[:4]}
    head['arguments'] = jsonArguments(result['arguments'])
    head['results_cwz'] = np.asarray(result['results_cwz'], dtype=np.float64).ravel().tolist()
    head['results_calls'] = [[int(c[0]), int(c[1]), int(c[2]), float(c[3]), float(c[4])] for c in calls]
    if strict:
        head = _json_nulls(head)
    return json.dumps(head, separators=(',', ':'), allow_nan=not strict)[:-1].encode('ascii')


def export_json_batch(results, strict=False, gz=False, device=0, ctx=None, max_rows=65535, details=None, max_bytes=4 << 30):
    """Result files as lossless JSON: a list of the files' bytes, one per result.  A file is one object with
    the keys JSON_KEYS in that order; the host writes everything up to results_calls (jsonHead), results_z and results_r
    are text the GPU writes (wc_json_rows_dev: CPython's own digits, so json.loads returns the stored doubles bit for
    bit).  strict: Infinity, -Infinity and NaN become null in both parts.  gz: the file is three gzip members in a row,
    the host part through zlib, `,"results_z":` + the z text and `,"results_r":` + the r text + `}` deflated on the GPU from
    the text where it lies (wc_deflate_rows_len_dev, one call for the rows of a GPU call, their lengths made on the
    device), from which only compressed bytes are copied.  results: dicts with JSON_KEYS' entries, results_z / results_r
    as per-chromosome arrays; all share the chromosome lengths.  A batch is split at max_rows rows and at max_bytes of
    device memory per GPU call.  details: a dict that receives 'times_ms' (per GPU call [copy in, text, deflate, copy
    out]) and 'text_bytes' (per file: z, r)."""
    import torch
    import zlib
    if not results:
        return []
    lib = _lib.load()
    sizes = np.array([len(c) for c in results[0]['results_z']], dtype=np.int64)
    for i, res in enumerate(results):
        for key in ('results_z', 'results_r'):
            if [len(c) for c in res[key]] != [int(v) for v in sizes]:
                raise ValueError('sample %d has other chromosome lengths in %s than the first has in results_z' % (i, key))
    bound = jsonRowBound(sizes)
    lead = 16                                   # room for the key in front of a row's text, which starts on a multiple of 16
    keys = (b',"results_z":', b',"results_r":')
    assert len(keys[0]) == len(keys[1]) <= lead

    def text_call(handle, stream, rows, row_stride, n_rows, text, text_stride, text_len, _):
        _lib.check(lib.wc_json_rows_dev(handle, stream, rows, row_stride, n_rows, _lib.ptr(sizes), len(sizes), int(bool(strict)), text,
                                        text_stride, text_len))

    def pack_call(handle, stream, text, counts, n, files):
        # the key goes in front of the text and the brace behind the r text, so a row is one gzip member's input; its
        # length is made on the device, and one call deflates the rows of both keys
        for k in range(2):
            text[k * n:(k + 1) * n, lead - len(keys[k]):lead] = torch.from_numpy(np.frombuffer(keys[k], dtype=np.uint8).copy()).to(text.device)
        text[torch.arange(n, 2 * n, device=text.device), lead + counts[0, n:].clamp(0, bound)] = ord('}')
        member = counts[0] + len(keys[0])
        member[n:] += 1
        _lib.check(lib.wc_deflate_rows_len_dev(handle, stream, text.data_ptr() + lead - len(keys[0]), 2 * n, member.data_ptr(),
                                               len(keys[0]) + bound + 1, text.shape[1], files.data_ptr(), files.shape[1],
                                               counts[2].data_ptr(), counts[3].data_ptr()))

    def piece(data, k, text_len, crc):
        return gzipAssemble(data, crc, len(keys[k]) + text_len + k) if gz else data.tobytes()

    pack = (len(keys[0]) + bound + 1, deflateBound(len(keys[0]) + bound + 1), 1, pack_call) if gz else None
    pieces, text_bytes, _ = _text_export_batch(results, ('z', 'r'), sizes, bound, lead, bound + 1, 2, text_call, pack, piece, device, ctx,
                                               max_rows, max_bytes, details)
    out = []
    for res, (z, r) in zip(results, pieces):
        head = jsonHead(res, strict)
        if gz:
            packer = zlib.compressobj(6, zlib.DEFLATED, -15)
            raw = packer.compress(head) + packer.flush()
            out.append(gzipAssemble(raw, zlib.crc32(head), len(head)) + z + r)
        else:
            out.append(head + keys[0] + z + keys[1] + r + b'}')
    if details is not None:
        details['text_bytes'] = text_bytes
    return out


# ------------------------------------------------------------------- exporttracks: bedGraph / BED ----
def _track_prefix(prefix):
    """The chromosome names' prefix as bytes: at most 16 ASCII bytes, no tab, no newline."""
    try:
        raw = prefix.encode('ascii') if isinstance(prefix, str) else bytes(prefix)
    except UnicodeEncodeError:
        raise ValueError('a chromosome prefix must be ASCII: %r' % (prefix,))
    if len(raw) > 16 or any(b in (0, 9, 10) or b > 127 for b in raw):
        raise ValueError('a chromosome prefix is at most 16 ASCII bytes without tab or newline: %r' % (prefix,))
    return raw


def bedgraphRowBound(sizes, binsize, prefix_len=3):
    """Most bytes the bedGraph text of one dense row takes (wc_bedgraph_row_bound; host only)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    bound = int(_lib.load().wc_bedgraph_row_bound(_lib.ptr(sizes), len(sizes), int(binsize), int(prefix_len)))
    if bound < 0:
        raise ValueError('bedgraphRowBound: unusable chromosome sizes, bin size or prefix')
    return bound


def bedgraphRows(rows, sizes, binsize, prefix='chr', clip=None, nozero=False, device=0, ctx=None, row_stride=None, times=None):
    """The bedGraph text of every dense float64 row (host array [n, >= sum(sizes)]), written on the GPU (wc_bedgraph_rows):
    (a list of bytes, the rows' counts of bins that are not finite).  clip: the chromosomes' lengths, or None.  times: a
    list that receives [copy in, lengths and scan, bytes, copy out] ms."""
    lib = _lib.load()
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    raw = _track_prefix(prefix)
    clip = None if clip is None else np.ascontiguousarray(clip, dtype=np.int64)
    n = rows.shape[0]
    stride = max(bedgraphRowBound(sizes, binsize, len(raw)), 1)
    text = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int64)
    dropped = np.zeros(n, dtype=np.int64)
    t_ms = np.zeros(4, dtype=np.float64) if times is not None else None
    _lib.check(lib.wc_bedgraph_rows(ctx or _lib.context(device), _lib.ptr(rows), int(rows.shape[1] if row_stride is None else row_stride), n,
                                    _lib.ptr(sizes), len(sizes), int(binsize), _lib.ptr(clip), raw, len(raw), int(bool(nozero)),
                                    _lib.ptr(text), stride, _lib.ptr(lens), _lib.ptr(dropped), _lib.ptr(t_ms)))
    if times is not None:
        times.extend(t_ms.tolist())
    return [text[i, :lens[i]].tobytes() for i in range(n)], dropped.tolist()


def callsBed(calls, binsize, prefix='chr', chrom_lengths=None, mineffect=0):
    """The calls of a result file as BED9 lines, as bytes (host only): one line per call [chromosome (from 1), first bin,
    last bin, z, effect] with abs(effect * 100) > mineffect (`report`'s rule), sorted by (chromosome, start, end), ties
    in the file's order.  The name column is z=%.2f;effect=%.2f%%, the score min(1000, round(|z| * 10)) (1000 for an
    infinite z, 0 for NaN), the colour 213,94,0 for a gain and 0,114,178 for a loss; ends are clipped to chrom_lengths."""
    name = _track_prefix(prefix).decode('ascii')
    binsize = int(binsize)
    lines = []
    for call in np.asarray(calls, dtype=np.float64).reshape(-1, 5):
        z, effect = float(call[3]), float(call[4])
        if not abs(effect * 100) > mineffect:
            continue
        chrom, start, end = int(call[0]), int(call[1]) * binsize, (int(call[2]) + 1) * binsize
        if chrom_lengths is not None and 1 <= chrom <= len(chrom_lengths):
            end = min(end, int(chrom_lengths[chrom - 1]))
        score = 0 if z != z else 1000 if z - z != 0 else min(1000, int(round(abs(z) * 10)))
        lines.append((chrom, start, end, '%s%d\t%d\t%d\tz=%.2f;effect=%.2f%%\t%d\t.\t%d\t%d\t%s\n'
                      % (name, chrom, start, end, z, effect * 100, score, start, end, '213,94,0' if effect > 0 else '0,114,178')))
    lines.sort(key=lambda line: line[:3])         # (stable: ties keep the file's order)
    return ''.join(line[3] for line in lines).encode('ascii')


TRACKS = ('z', 'r')


def export_tracks_batch(results, only=None, gz=False, nozero=False, prefix='chr', chrom_lengths=None, device=0, ctx=None, details=None,
                        mineffect=0, max_rows=65535, max_bytes=4 << 30):
    """Result files as genome browser tracks: per result a tuple of the files' bytes, the bedGraph text of
    results_z and of results_r (`only`: 'z' or 'r' alone) and the calls as BED9 (callsBed, on the host).  A track has one
    line per run of bins with the same bits inside a chromosome, written by the GPU (wc_bedgraph_rows_dev); with gz it
    is BGZF, made from the text where it lies (wc_bgzf_rows_dev, one call for the rows of a GPU call, their lengths read
    on the device), and only the compressed bytes are copied.  results: dicts with binsize, results_z, results_r,
    results_calls; all share the chromosome lengths and the bin size.  chrom_lengths: the chromosomes' lengths in bases
    (ends are clipped to them), or None.  mineffect: callsBed's.  A batch is split at max_rows rows and at max_bytes of device memory per GPU
    call.  details: a dict that receives 'times_ms' (per GPU call [copy in, text, BGZF, copy out]), 'text_bytes' (per file
    and track), 'dropped' (per file and track: bins that are not finite)."""
    if only not in (None,) + TRACKS:
        raise ValueError("only: 'z', 'r' or None, not %r" % (only,))
    if not results:
        return []
    lib = _lib.load()
    which = [k for k in TRACKS if only in (None, k)]
    raw = _track_prefix(prefix)
    binsize = int(results[0]['binsize'])
    sizes = np.array([len(c) for c in results[0]['results_z']], dtype=np.int64)
    for i, res in enumerate(results):
        if int(res['binsize']) != binsize or res['binsize'] != binsize:
            raise ValueError('sample %d has bin size %s, the first has %s' % (i, res['binsize'], binsize))
    clip = None
    if chrom_lengths is not None:
        clip = np.ascontiguousarray(chrom_lengths, dtype=np.int64)
        if len(clip) != len(sizes):
            raise ValueError('%d chromosome lengths for %d chromosomes' % (len(clip), len(sizes)))
    bound = bedgraphRowBound(sizes, binsize, len(raw))

    def text_call(handle, stream, rows, row_stride, n_rows, text, text_stride, text_len, dropped):
        _lib.check(lib.wc_bedgraph_rows_dev(handle, stream, rows, row_stride, n_rows, _lib.ptr(sizes), len(sizes), binsize, _lib.ptr(clip),
                                            raw, len(raw), int(bool(nozero)), text, text_stride, text_len, dropped))

    def pack_call(handle, stream, text, counts, n, files):
        _lib.check(lib.wc_bgzf_rows_dev(handle, stream, text.data_ptr(), text.shape[0], counts[0].data_ptr(), bound, text.shape[1],
                                        files.data_ptr(), files.shape[1], counts[2].data_ptr()))

    pack = (bound, int(lib.wc_bgzf_bound(bound)), 28, pack_call) if gz else None
    pieces, text_bytes, dropped_bins = _text_export_batch(results, which, sizes, bound, 0, bound, 0, text_call, pack,
                                                          lambda data, k, text_len, crc: data.tobytes(), device, ctx, max_rows,
                                                          max_bytes, details)
    if details is not None:
        details['text_bytes'] = text_bytes
        details['dropped'] = dropped_bins
    return [files + (callsBed(res['results_calls'], binsize, prefix=prefix, chrom_lengths=chrom_lengths, mineffect=mineffect),)
            for res, files in zip(results, pieces)]


# ---------------------------------------------------------------------------
# sensitivity: thin mirrors of sensitivity.py, which imports this module
# ---------------------------------------------------------------------------
def spikeCounts(base, chrom_sizes, plan, device=0, draw=False, seed=1, trial0=0):
    from . import sensitivity
    return sensitivity.spikeCounts(base, chrom_sizes, plan, device=device, draw=draw, seed=seed, trial0=trial0)


def thinCounts(base, chrom_sizes, keep_ppm, seed=1, device=0):
    from . import sensitivity
    return sensitivity.thinCounts(base, chrom_sizes, keep_ppm, seed=seed, device=device)


def scoreTrials(plan, calls, n_calls, device=0):
    from . import sensitivity
    return sensitivity.scoreTrials(plan, calls, n_calls, device=device)


def makePlan(reference, n_samples, lengths_bins, effects_ppm, trials, chromosomes=None, seed=1, n_depths=1):
    from . import sensitivity
    return sensitivity.makePlan(reference, n_samples, lengths_bins, effects_ppm, trials, chromosomes=chromosomes, seed=seed,
                                n_depths=n_depths)


def sensitivityTable(plan, rec_i, rec_f, lengths_bins, effects_ppm, minoverlap=0.5, depths_ppm=None, n_samples=None):
    from . import sensitivity
    return sensitivity.sensitivityTable(plan, rec_i, rec_f, lengths_bins, effects_ppm, minoverlap=minoverlap, depths_ppm=depths_ppm,
                                        n_samples=n_samples)


def sensitivity_batch(reference, samples, plan, threshold, **options):
    from . import sensitivity
    return sensitivity.sensitivity_batch(reference, samples, plan, threshold, **options)
