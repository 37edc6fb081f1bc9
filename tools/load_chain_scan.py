#!/usr/bin/env python3
"""Dependent load chains in a gfx950 assembly listing: a wave that waits for ONE load at a time pays a memory round trip
per load, where a batch of loads in front of one wait pays a single trip.  Per kernel this reports, in text order,

  * every `s_waitcnt vmcnt(0)` with exactly one vector load (global / flat / buffer / scratch) issued since the previous
    wait on vmcnt (or the kernel's entry): a lone round trip;
  * every loop (a label and a later branch back to it) that holds a vector load and such a wait: a round trip per
    iteration.

Text order is not execution order: a wait at the head of a block that several paths reach is counted with the loads of
the text in front of it.  The figures compare two builds of one source; they are not a cycle count.

    python tools/load_chain_scan.py file.s [kernel substring ...]   -> one line per kernel, then its findings
"""
import re
import sys

LOAD = re.compile(r"^(global|flat|buffer|scratch)_load_")
LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
BRANCH = re.compile(r"^s_c?branch\w*\s+(\.L[\w.$]+)")
VMCNT = re.compile(r"vmcnt\((\d+)\)")


def short_name(symbol):
    """k_pick out of _ZN12_GLOBAL__N_16k_pickENS_8PickArgsE (template arguments are dropped)."""
    s = symbol
    if s.startswith("_ZN12_GLOBAL__N_1"):
        s = s[len("_ZN12_GLOBAL__N_1"):]
    elif s.startswith("_Z"):
        s = s[2:].lstrip("N")
    m = re.match(r"(\d+)", s)
    if not m:
        return symbol
    n = int(m.group(1))
    return s[m.end():m.end() + n]


def scan(path):
    """-> {symbol: {"waits": [(line, load line, load text)], "loops": [(label, first line, last line, loads, waits)]}}
    for every function of the listing that ends in s_endpgm."""
    out = {}
    kernel = None
    cur = None
    for no, raw in enumerate(open(path, errors="ignore"), 1):
        t = raw.split(";")[0].strip()
        if not t:
            continue
        m = LABEL.match(t)
        if m:
            name = m.group(1)
            if name.startswith(".L"):
                if cur is not None:
                    cur["labels"][name] = no
            else:
                kernel = name
                cur = {"waits": [], "loops": [], "labels": {}, "loads": [], "since": [], "ended": False}
                out[kernel] = cur
            continue
        if t.startswith(".") or cur is None or cur["ended"]:
            continue
        op = t.split()[0]
        if LOAD.match(op):
            cur["loads"].append(no)
            cur["since"].append((no, t))
        elif op == "s_waitcnt":
            m = VMCNT.search(t)
            if m:
                if int(m.group(1)) == 0 and len(cur["since"]) == 1:
                    cur["waits"].append((no, cur["since"][0][0], cur["since"][0][1]))
                cur["since"] = []
        elif op == "s_endpgm":
            cur["ended"] = True
        else:
            m = BRANCH.match(t)
            if m and m.group(1) in cur["labels"]:           # a branch back: the label is above it in the text
                first = cur["labels"][m.group(1)]
                loads = [ln for ln in cur["loads"] if first < ln < no]
                waits = [w[0] for w in cur["waits"] if first < w[0] < no]
                if loads and waits:
                    # (several branches back to one label are one loop: the last one spans it)
                    cur["loops"] = [lp for lp in cur["loops"] if lp[0] != m.group(1)]
                    cur["loops"].append((m.group(1), first, no, len(loads), len(waits)))
    return {k: {"waits": v["waits"], "loops": v["loops"]} for k, v in out.items() if v["ended"]}


def counts(path):
    """-> {short kernel name: (lone waits, loops with a load and a lone wait)}, template instances summed."""
    res = {}
    for sym, r in scan(path).items():
        name = short_name(sym)
        w, l = res.get(name, (0, 0))
        res[name] = (w + len(r["waits"]), l + len(r["loops"]))
    return res


def report(path, only=()):
    lines = []
    for sym, r in scan(path).items():
        name = short_name(sym)
        if only and not any(o in name for o in only):
            continue
        lines.append("%-22s lone waits %3d   loops with a load and a lone wait %2d   (%s)"
                     % (name, len(r["waits"]), len(r["loops"]), sym[:60]))
        for no, lno, text in r["waits"]:
            lines.append("      line %6d waits for line %6d: %s" % (no, lno, " ".join(text.split())[:70]))
        for label, first, last, nl, nw in r["loops"]:
            lines.append("      loop %s lines %d-%d: %d loads, %d lone waits" % (label, first, last, nl, nw))
    return lines


if __name__ == "__main__":
    print("\n".join(report(sys.argv[1], sys.argv[2:])))
