#!/usr/bin/env python
"""Writes wisecondor_amd/csrc/fmt_double_tab.h: the 128-bit multiples of powers of 5 that fmt_double.h multiplies by.

    python tools/make_fmt_tables.py            rewrite the header
    python tools/make_fmt_tables.py --check    exit status 1 if the committed header is not what this script writes

Everything is Python integer arithmetic, so every entry is exact:
  FD_POW5_INV[q] = floor(2^(bits(5^q) - 1 + 125) / 5^q) + 1     q = 0 .. 341   (the reciprocal, rounded up)
  FD_POW5[i]     = 5^i shifted to exactly 125 bits (towards zero) i = 0 .. 325
as (low, high) pairs of 64-bit words.  bits(x) is x.bit_length().
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "wisecondor_amd", "csrc", "fmt_double_tab.h")
BITS = 125
N_INV, N_POW = 342, 326
MASK = (1 << 64) - 1


def tables():
    inv, pw = [], []
    for q in range(N_INV):
        p = 5 ** q
        inv.append((1 << (p.bit_length() - 1 + BITS)) // p + 1)
    for i in range(N_POW):
        p = 5 ** i
        shift = p.bit_length() - BITS
        pw.append(p >> shift if shift >= 0 else p << -shift)
    return inv, pw


def text():
    inv, pw = tables()
    lines = ["// Written by tools/make_fmt_tables.py; do not edit.  (low, high) words of the 128-bit multipliers of fmt_double.h.",
             "#pragma once",
             "#define FD_POW5_BITS %d" % BITS,
             "#define FD_N_POW5_INV %d" % N_INV,
             "#define FD_N_POW5 %d" % N_POW,
             "#define FD_POW5_INV_ROWS \\"]
    for v in inv:
        assert v < 1 << 128
        lines.append("    {0x%016xull, 0x%016xull}, \\" % (v & MASK, v >> 64))
    lines[-1] = lines[-1][:-2]
    lines.append("")
    lines.append("#define FD_POW5_ROWS \\")
    for v in pw:
        assert v.bit_length() == BITS
        lines.append("    {0x%016xull, 0x%016xull}, \\" % (v & MASK, v >> 64))
    lines[-1] = lines[-1][:-2]
    lines.append("")
    return "\n".join(lines)


if __name__ == "__main__":
    if "--check" in sys.argv:
        with open(OUT) as f:
            sys.exit(0 if f.read() == text() else 1)
    with open(OUT, "w") as f:
        f.write(text())
    print(OUT)
