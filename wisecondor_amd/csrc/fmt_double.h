// The text CPython's float.__repr__ (and so json.dumps) gives for a double, made from the 64 bits by integer arithmetic
// alone; one routine for the host and the device.
//
// The digits are Ryu's (Ulf Adams, "Ryu: fast float-to-string conversion", PLDI 2018): with the double v = m2 * 2^e2 and
// its two neighbours' halfway points, all three are scaled by a power of 10 such that the digits of the products'
// integer parts are decimal digits of the values; the shortest number inside the interval is found by dropping digits
// from all three until the bounds meet, and the last digit is rounded to the nearest, a tie to even.  The scaling is a
// multiplication by a 125-bit multiple of a power of 5 (fmt_double_tab.h, which tools/make_fmt_tables.py writes) and a
// shift; the paper proves that 125 bits leave the integer part exact for every double, and whether the dropped part was
// exactly zero, which decides the ties and the closed bounds, is tested separately by divisibility.  So every value is
// exact; there is no floating-point operation and no approximate path.
//
//   fd_decimal(bits)        the class, the sign, and for a finite non-zero value the digits as an integer of 1 .. 17 digits
//                           and the power of 10 of its last digit
//   fd_length(d, strict)    bytes of the text, 1 .. 24
//   fd_write(d, strict, p)  the text at p (no terminator), returns its length.  p[k] is stored at computed k: p may be
//                           LDS, and nothing here is an array in registers
// The form is repr's: positional while -4 < decimal point <= 16, else d[.ddd]e+XX with at least two exponent digits;
// whole numbers get ".0"; -0.0 keeps its sign.  Not finite: Infinity, -Infinity, NaN (any sign, any payload), as
// json.dumps writes them, or null for all three when strict.
#pragma once
#include <stdint.h>

#include "fmt_double_tab.h"

#if defined(__HIPCC__)
#define FD_HD __host__ __device__
#else
#define FD_HD
#endif

#define FD_MAX_TEXT 24

static const uint64_t fd_pow5_inv_host[FD_N_POW5_INV][2] = {FD_POW5_INV_ROWS};
static const uint64_t fd_pow5_host[FD_N_POW5][2] = {FD_POW5_ROWS};
#if defined(__HIPCC__)
static __device__ const uint64_t fd_pow5_inv_dev[FD_N_POW5_INV][2] = {FD_POW5_INV_ROWS};
static __device__ const uint64_t fd_pow5_dev[FD_N_POW5][2] = {FD_POW5_ROWS};
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define FD_POW5_INV fd_pow5_inv_dev
#define FD_POW5 fd_pow5_dev
#else
#define FD_POW5_INV fd_pow5_inv_host
#define FD_POW5 fd_pow5_host
#endif

enum { FD_FINITE = 0, FD_ZERO = 1, FD_INF = 2, FD_NAN = 3 };

struct FdDec {
    uint64_t digits;    // FD_FINITE: the decimal digits as an integer, 1 .. 17 of them
    int32_t exp;        // FD_FINITE: value = digits * 10^exp
    uint32_t kind;      // bits 0 .. 1 the class, bit 31 the sign
};

// bits of 5^e, e <= 3528;  floor(log10(2^e)), e <= 1650;  floor(log10(5^e)), e <= 2620
FD_HD inline int32_t fd_pow5bits(int32_t e) { return (int32_t)(((uint32_t)e * 1217359u) >> 19) + 1; }
FD_HD inline int32_t fd_log10pow2(int32_t e) { return (int32_t)(((uint32_t)e * 78913u) >> 18); }
FD_HD inline int32_t fd_log10pow5(int32_t e) { return (int32_t)(((uint32_t)e * 732923u) >> 20); }

// is 5^p a divisor of v (v != 0)
FD_HD inline bool fd_multiple_of_pow5(uint64_t v, int32_t p) {
    int32_t count = 0;
    for (;;) {
        const uint64_t q = v / 5u;
        if (v - 5u * q != 0) break;
        v = q;
        ++count;
    }
    return count >= p;
}

// floor(m * mul / 2^j), mul = mul[0] + 2^64 mul[1], 64 <= j < 192: the low 64 bits of the product cannot reach the result
FD_HD inline uint64_t fd_mulshift(uint64_t m, const uint64_t *mul, int32_t j) {
    const unsigned __int128 b0 = (unsigned __int128)m * mul[0];
    const unsigned __int128 b2 = (unsigned __int128)m * mul[1];
    return (uint64_t)(((b0 >> 64) + b2) >> (j - 64));
}

FD_HD inline int fd_digits_of(uint64_t v) {      // v < 10^17
    int n = 1;
    if (v >= 10000000000000000ull) return 17;
    if (v >= 100000000ull) { v /= 100000000ull; n += 8; }
    if (v >= 10000u) { v /= 10000u; n += 4; }
    if (v >= 100u) { v /= 100u; n += 2; }
    if (v >= 10u) n += 1;
    return n;
}

FD_HD inline FdDec fd_decimal(uint64_t bits) {
    FdDec d;
    const uint64_t frac = bits & ((1ull << 52) - 1);
    const uint32_t bexp = (uint32_t)(bits >> 52) & 0x7ffu;
    const uint32_t sign = (uint32_t)(bits >> 63) << 31;
    d.digits = 0;
    d.exp = 0;
    if (bexp == 0x7ffu) {
        d.kind = frac ? (uint32_t)FD_NAN : (sign | FD_INF);
        return d;
    }
    if (bexp == 0 && frac == 0) {
        d.kind = sign | FD_ZERO;
        return d;
    }
    d.kind = sign | FD_FINITE;
    // v = m2 * 2^e2 with two extra bits, so that the halfway points to the neighbours are integers: 4 m2 + 2 above and
    // 4 m2 - 2 below (4 m2 - 1 where the lower neighbour is half as far away: at a power of two)
    int32_t e2;
    uint64_t m2;
    if (bexp == 0) {
        e2 = 1 - 1023 - 52 - 2;
        m2 = frac;
    } else {
        e2 = (int32_t)bexp - 1023 - 52 - 2;
        m2 = (1ull << 52) | frac;
    }
    const bool accept = (m2 & 1u) == 0;         // a round-half-even reader takes the bounds themselves for an even m2
    const uint64_t mv = 4 * m2;
    const uint32_t mm_shift = frac != 0 || bexp <= 1;
    uint64_t vr, vp, vm;
    int32_t e10;
    bool vm_zeros = false, vr_zeros = false;     // everything dropped so far from vm / vr was zero
    if (e2 >= 0) {
        const int32_t q = fd_log10pow2(e2) - (e2 > 3);
        e10 = q;
        const int32_t k = FD_POW5_BITS + fd_pow5bits(q) - 1;
        const int32_t j = -e2 + q + k;
        const uint64_t *mul = FD_POW5_INV[q];
        vr = fd_mulshift(mv, mul, j);
        vp = fd_mulshift(mv + 2, mul, j);
        vm = fd_mulshift(mv - 1 - mm_shift, mul, j);
        if (q <= 21) {                           // (only then can a number below 2^57 be a multiple of 5^q)
            if (mv % 5u == 0) vr_zeros = fd_multiple_of_pow5(mv, q);
            else if (accept) vm_zeros = fd_multiple_of_pow5(mv - 1 - mm_shift, q);
            else vp -= fd_multiple_of_pow5(mv + 2, q);
        }
    } else {
        const int32_t q = fd_log10pow5(-e2) - (-e2 > 1);
        e10 = q + e2;
        const int32_t i = -e2 - q;
        const int32_t k = fd_pow5bits(i) - FD_POW5_BITS;
        const int32_t j = q - k;
        const uint64_t *mul = FD_POW5[i];
        vr = fd_mulshift(mv, mul, j);
        vp = fd_mulshift(mv + 2, mul, j);
        vm = fd_mulshift(mv - 1 - mm_shift, mul, j);
        if (q <= 1) {
            vr_zeros = true;                     // mv = 4 m2 always has two trailing zero bits
            if (accept) vm_zeros = mm_shift == 1;
            else --vp;
        } else if (q < 63) {
            vr_zeros = (mv & ((1ull << q) - 1)) == 0;
        }
    }
    int32_t removed = 0;
    uint32_t last = 0;
    uint64_t out;
    if (vm_zeros || vr_zeros) {
        while (vp / 10u > vm / 10u) {
            vm_zeros &= vm % 10u == 0;
            vr_zeros &= last == 0;
            last = (uint32_t)(vr % 10u);
            vr /= 10u; vp /= 10u; vm /= 10u;
            ++removed;
        }
        if (vm_zeros) {
            while (vm % 10u == 0) {
                vr_zeros &= last == 0;
                last = (uint32_t)(vr % 10u);
                vr /= 10u; vp /= 10u; vm /= 10u;
                ++removed;
            }
        }
        if (vr_zeros && last == 5 && vr % 2u == 0) last = 4;      // exactly halfway: to even
        out = vr + ((vr == vm && (!accept || !vm_zeros)) || last >= 5);
    } else {
        bool up = false;
        while (vp / 10u > vm / 10u) {
            up = vr % 10u >= 5;
            vr /= 10u; vp /= 10u; vm /= 10u;
            ++removed;
        }
        out = vr + (vr == vm || up);
    }
    d.digits = out;
    d.exp = e10 + removed;
    return d;
}

// the layout of a finite non-zero value: n digits, the decimal point's place decpt (value = 0.ddd * 10^decpt)
FD_HD inline int fd_length(const FdDec &d, int strict) {
    const int cls = (int)(d.kind & 3u), neg = (int)(d.kind >> 31);
    if (cls == FD_NAN) return strict ? 4 : 3;
    if (cls == FD_INF) return strict ? 4 : 8 + neg;
    if (cls == FD_ZERO) return 3 + neg;
    const int n = fd_digits_of(d.digits), decpt = d.exp + n;
    if (decpt > -4 && decpt <= 16) return neg + (decpt <= 0 ? 2 - decpt + n : decpt >= n ? decpt + 2 : n + 1);
    const int e = decpt - 1, a = e < 0 ? -e : e;
    return neg + n + (n > 1) + 2 + (a >= 100 ? 3 : 2);
}

FD_HD inline int fd_write(const FdDec &d, int strict, unsigned char *p) {
    const int cls = (int)(d.kind & 3u), neg = (int)(d.kind >> 31);
    if (cls >= FD_INF) {
        const char *s = strict ? "null" : cls == FD_NAN ? "NaN" : neg ? "-Infinity" : "Infinity";
        int k = 0;
        for (; s[k]; ++k) p[k] = (unsigned char)s[k];
        return k;
    }
    if (neg) *p++ = '-';
    if (cls == FD_ZERO) {
        p[0] = '0'; p[1] = '.'; p[2] = '0';
        return neg + 3;
    }
    const int n = fd_digits_of(d.digits), decpt = d.exp + n;
    uint64_t v = d.digits;
    int first, dot, len;        // digit i stands at first + i + (i >= dot)
    if (decpt > -4 && decpt <= 16) {
        if (decpt <= 0) {
            p[0] = '0'; p[1] = '.';
            for (int k = 0; k < -decpt; ++k) p[2 + k] = '0';
            first = 2 - decpt; dot = n; len = first + n;
        } else if (decpt >= n) {
            for (int k = n; k < decpt; ++k) p[k] = '0';
            p[decpt] = '.'; p[decpt + 1] = '0';
            first = 0; dot = n; len = decpt + 2;
        } else {
            p[decpt] = '.';
            first = 0; dot = decpt; len = n + 1;
        }
    } else {
        const int e = decpt - 1, a = e < 0 ? -e : e;
        int at = n;
        if (n > 1) { p[1] = '.'; ++at; }
        p[at++] = 'e';
        p[at++] = e < 0 ? '-' : '+';
        if (a >= 100) p[at++] = (unsigned char)('0' + a / 100);
        p[at++] = (unsigned char)('0' + a / 10 % 10);
        p[at++] = (unsigned char)('0' + a % 10);
        first = 0; dot = 1; len = at;
    }
    for (int i = n - 1; i >= 0; --i) {
        p[first + i + (i >= dot)] = (unsigned char)('0' + (int)(v % 10u));
        v /= 10u;
    }
    return neg + len;
}
