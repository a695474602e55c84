"""ISA lint of the generated gfx950 code: the store order behind a completion stamp.

Single-instance handles read their answer from pinned host memory by polling a completion stamp (tinympc_synchronize,
wait_session_solution). The kernels of layouts C and F write that answer with host_store() -- relaxed system-scope stores, written through
(`sc0 sc1`) -- from every wavefront, then raise the stamp: every thread retires its own stores (host_stores_retired: s_waitcnt vmcnt(0)),
the workgroup meets at a barrier, one thread stores the stamp (host_stamp_store; all three in tinympc_device.h). A stamp that can overtake
a store still in flight is a stale read on the host that no run-time test pins: the window is a few hundred nanoseconds. Through round 5
the wait was believed to come with a workgroup-scope release fence, which emits none; this lint checks the generated code instead.

`lint(asm_text)` -> ({kernel function: number of stamp sites}, violations). The two helpers leave fixed comments in the assembly
(STAMP_MARK, WAIT_MARK); a stamp site is the s_barrier in front of a STAMP_MARK, found by walking back from the mark. From the barrier
the lint walks back along EVERY path that reaches it (a label is followed to the branches that jump to it, as tools/isa_lint.py does, and
straight up unless nothing falls through into it):
  1. an s_waitcnt whose operands contain vmcnt(0) must be met before any host store (a global_ / flat_ / buffer_store with sc0 AND sc1) is.
     The write-out's stores sit in loops whose bodies begin with a vmcnt(0) for a load: the first wait in program order proves nothing,
     the loop's exit path is what counts -- hence the walk.
  2. no buffer_wbl2 and no buffer_inv between the last host stores in front of the barrier and the stamp: the write-through stores
     exist so that the L2 is neither written back nor invalidated once per tick (what an agent- or system-scope fence would add).
  3. the function contains WAIT_MARK: the wait is the helper's, not one the compiler happened to need for a load.
Host stores that are NOT followed by a wait -- layout F's early-answer lines (SolveParams::host_ans), which check themselves -- are no
finding: only what precedes a stamp's barrier is looked at. The lint looks for store, wait, barrier and cache write-back / invalidate
mnemonics and for the two marks, nothing else.

Used by __graft_entry__.build() on the assembly of the objects it links (a violation fails the build) and by tests/test_stamp_order.py.
    python tools/stamp_lint.py file.s ..."""
from __future__ import annotations

import os
import re
import sys

if __package__ in (None, ""):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.isa_lint import NO_FALL_THROUGH, parse

WAIT_MARK = "tinympc host stores retired"   # host_stores_retired(), tinympc_device.h
STAMP_MARK = "tinympc completion stamp"     # host_stamp_store()
VMCNT0 = re.compile(r"\bvmcnt\(0\)")
CACHE_OPS = ("buffer_wbl2", "buffer_inv")
INDIRECT = ("s_setpc_b64", "s_swappc_b64")


def _text(it) -> str:
    return it[6].split(";")[0]


def is_host_store(it) -> bool:
    if not it[1].startswith(("global_store", "flat_store", "buffer_store")):
        return False
    words = _text(it).replace(",", " ").split()
    return "sc0" in words and "sc1" in words


def is_retiring_wait(it) -> bool:
    return it[1] == "s_waitcnt" and bool(VMCNT0.search(_text(it)))


def functions(items):
    """-> [(name, lo, hi)]: the item ranges of the functions, `name:` ... `.Lfunc_end` (data symbols and the metadata's keys are labels too,
    but nothing closes them). Text without any `.Lfunc_end` (planted text in tests) is one function named ""."""
    out, name, lo = [], None, 0
    for i, it in enumerate(items):
        if it[0] != "label":
            continue
        if it[1].startswith(".Lfunc_end"):
            if name is not None:
                out.append((name, lo, i))
            name = None
        elif not it[1].startswith(".L"):
            name, lo = it[1], i + 1
    if not out and not any(it[0] == "label" and it[1].startswith(".Lfunc_end") for it in items):
        out.append(("", 0, len(items)))
    return out


def _walk_back(items, sites, lo, hi, start, state, step):
    """Walks back from item `start` (inclusive) along every path that reaches it inside [lo, hi). step(state, index, item) returns the
    state to go on with, or None where the path ends; it is called with item None where a path reaches the function's first instruction."""
    seen, stack = set(), [(start, state)]
    while stack:
        i, st = stack.pop()
        while True:
            if i < lo:
                step(st, i, None)
                break
            if (i, st) in seen:
                break
            seen.add((i, st))
            it = items[i]
            if it[0] == "label":
                stack.extend((b, st) for b in sites.get(it[1], []) if lo <= b < hi)
                i -= 1
                if i >= lo and items[i][0] == "instr" and items[i][1] in NO_FALL_THROUGH:
                    break  # nothing falls through into the label
                continue
            st = step(st, i, it)
            if st is None:
                break
            i -= 1


def lint(asm_text: str):
    """Returns ({function name: number of stamp sites}, list of violations (line, instruction text, reason))."""
    items, sites = parse(asm_text, marks=(WAIT_MARK, STAMP_MARK))
    counts, bad = {}, []

    def report(it, why):
        v = (it[5], it[6], why)
        if v not in bad:
            bad.append(v)

    for name, lo, hi in functions(items):
        stamps = [i for i in range(lo, hi) if items[i][0] == "instr" and items[i][1] == STAMP_MARK]
        counts[name] = len(stamps)
        if stamps and not any(items[i][0] == "instr" and items[i][1] == WAIT_MARK for i in range(lo, hi)):
            report(items[stamps[0]], "%s: a stamp is raised without host_stores_retired()" % name)
        for m in stamps:
            mark = items[m]
            # the stamp itself: the first thing behind the mark that is not plain arithmetic must be a host store
            j = m + 1
            while j < hi and items[j][0] == "instr" and not is_host_store(items[j]) and items[j][1] != "s_barrier" and not items[j][4] and items[j][1] not in NO_FALL_THROUGH:
                if items[j][1].startswith(CACHE_OPS):
                    report(items[j], "%s: %s between the barrier and the stamp at line %d" % (name, items[j][1], mark[5]))
                j += 1
            if not (j < hi and items[j][0] == "instr" and is_host_store(items[j])):
                report(mark, "%s: no write-through store behind the stamp's mark" % name)
            # the site: the barrier in front of the stamp, on every path
            barriers = []

            def to_barrier(st, i, it):
                if it is None:
                    report(mark, "%s: a path reaches the stamp without a barrier" % name)
                    return None
                if it[1] == "s_barrier":
                    if i not in barriers:
                        barriers.append(i)
                    return None
                if it[1].startswith(CACHE_OPS):
                    report(it, "%s: %s between the barrier and the stamp at line %d" % (name, it[1], mark[5]))
                if it[1] in INDIRECT:
                    report(it, "%s: indirect branch between the barrier and the stamp at line %d" % (name, mark[5]))
                    return None
                return st

            _walk_back(items, sites, lo, hi, m - 1, 0, to_barrier)

            # in front of the barrier: state 0 = no retiring wait met yet on this path, 1 = met (the walk goes on to the last host stores)
            def to_stores(st, i, it):
                if it is None:
                    return None  # the function's start: no host store on this path at all
                if it[1].startswith(CACHE_OPS):
                    report(it, "%s: %s between the last host stores and the stamp at line %d" % (name, it[1], mark[5]))
                    return st
                if it[1] in INDIRECT:
                    report(it, "%s: indirect branch in front of the stamp's barrier (stamp at line %d)" % (name, mark[5]))
                    return None
                if is_host_store(it):
                    if st == 0:
                        report(it, "%s: host store with no s_waitcnt vmcnt(0) between it and the barrier of the stamp at line %d" % (name, mark[5]))
                    return None
                if st == 0 and is_retiring_wait(it):
                    return 1
                if st == 1 and it[1] == "s_barrier":
                    return None  # an earlier phase of the kernel
                return st

            for b in barriers:
                _walk_back(items, sites, lo, hi, b - 1, 0, to_stores)
    return counts, bad


def lint_file(path: str):
    with open(path) as f:
        return lint(f.read())


if __name__ == "__main__":
    rc = 0
    for p in sys.argv[1:]:
        counts, bad = lint_file(p)
        print("%s: %d function(s), %d with a stamp site, %d violation(s)" % (p, len(counts), sum(1 for n in counts.values() if n), len(bad)))
        for n, c in counts.items():
            if c == 0:
                print("  no stamp: %s" % n)
        for ln, text, why in bad[:40]:
            print("  line %d: %s\n      %s" % (ln, text, why))
        rc |= bool(bad)
    sys.exit(rc)
