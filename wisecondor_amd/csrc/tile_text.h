// What the text kernels of export.hip and tracks.hip share: a row's text is made tile by tile, a workgroup of TT_T lanes
// per tile and a lane per value; the lanes' byte counts are summed inside the tile, every lane writes its bytes into the
// tile's image in LDS, and the image leaves in aligned 16-byte lines.
#pragma once
#include "common.h"

const int TT_T = 256;                   // values per tile = lanes per workgroup

// the chromosome of value j (0 <= j < off[n_chrom]): the last one that starts at or before j and is not empty
__device__ __forceinline__ int tt_chrom_of(const long long *off, int n_chrom, long long j) {
    int lo = 0, hi = n_chrom;           // off[lo] <= j < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= j) lo = mid;
        else hi = mid;
    }
    return lo;
}

// inclusive sum over the workgroup's lanes (buf: TT_T ints); every lane calls it
__device__ __forceinline__ int tt_scan(int v, int *buf) {
    const int t = threadIdx.x;
    buf[t] = v;
    wc_sync();
    for (int step = 1; step < TT_T; step <<= 1) {
        const int add = t >= step ? buf[t - step] : 0;
        wc_sync();
        buf[t] += add;
        wc_sync();
    }
    return buf[t];
}

// image[g - a0] for the global bytes g of [r0, r1), a0 = r0 rounded down to 16: whole lines as 16-byte stores, the
// parts of the first and the last line byte by byte (`out` + a0 is 16-byte aligned)
__device__ __forceinline__ void tt_store(const unsigned char *image, long long a0, long long r0, long long r1, unsigned char *out) {
    for (int line = threadIdx.x; a0 + 16ll * line < r1; line += TT_T) {
        const long long g = a0 + 16ll * line;
        if (g >= r0 && g + 16 <= r1) {
            *reinterpret_cast<uint4 *>(out + g) = reinterpret_cast<const uint4 *>(image)[line];
        } else {
            const long long from = g > r0 ? g : r0, to = g + 16 < r1 ? g + 16 : r1;
            for (long long q = from; q < to; ++q) out[q] = image[q - a0];
        }
    }
}
