#!/usr/bin/env python3
"""Do two builds enqueue the same work in the same order?  Compares two rocprofv3 --kernel-trace --memory-copy-trace runs
(rocpd databases, as tools/kernel_avgs.py reads) of one workload:

  * per process and queue, the ordered list of (kernel name, grid, workgroup) -- the runs' own queue ids do not matter, and
    a kernel that moved to another queue shows as a difference;
  * per process and queue, the ordered list of copies (direction, bytes).

usage: trace_compare.py <label> <dir or .db of run A> <dir or .db of run B>
Prints one summary line per comparison and the first differences; exit status 1 when the runs differ.
"""
import glob
import os
import sqlite3
import sys


def _dbs(path):
    if os.path.isfile(path):
        return [path]
    return sorted(glob.glob(os.path.join(path, "**", "*.db"), recursive=True))


def _by_queue(rows):
    """rows: (pid, queue id, start, item) -> {process number: the queues' ordered lists of items, sorted by content}.
    Processes are numbered by first use; queues carry no number at all -- which hardware queue a stream gets, and which of two
    host threads dispatches first, differ from run to run -- so two runs agree when their queues hold the same lists."""
    pids, lists = {}, {}
    for pid, q, _, item in sorted(rows, key=lambda r: r[2]):
        lists.setdefault((pids.setdefault(pid, len(pids)), q), []).append(item)
    out = {}
    for (p, _), items in lists.items():
        out.setdefault(p, []).append(items)
    return {p: sorted(v, key=repr) for p, v in out.items()}


def load(path):
    kernels, copies = [], []
    for db in _dbs(path):
        c = sqlite3.connect(db)
        kernels += [(pid, q, start, (name, (gx, gy, gz), (wx, wy, wz))) for pid, q, start, name, gx, gy, gz, wx, wy, wz in
                    c.execute("select pid, queue_id, start, name, grid_x, grid_y, grid_z, workgroup_x, workgroup_y, "
                              "workgroup_z from kernels")]
        try:
            copies += [(pid, q, start, (name, size)) for pid, q, start, name, size in
                       c.execute("select pid, queue_id || '/' || stream_id, start, name, size from memory_copies")]
        except sqlite3.OperationalError:  # a run without a single copy has no such view
            pass
    return _by_queue(kernels), _by_queue(copies)


def compare(what, a, b):
    same = True
    for p in sorted(set(a) | set(b)):
        qa, qb = a.get(p, []), b.get(p, [])
        if len(qa) != len(qb):
            same = False
            print("  %s, process %d: DIFFER, %d vs %d queues" % (what, p, len(qa), len(qb)))
            continue
        for n, (la, lb) in enumerate(zip(qa, qb)):
            if la == lb:
                print("  %s, process %d queue %d: %d entries, equal" % (what, p, n, len(la)))
                continue
            same = False
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            print("  %s, process %d queue %d: DIFFER (%d vs %d entries), first at %d:" % (what, p, n, len(la), len(lb), i))
            print("    A: %r" % (la[i:i + 3],))
            print("    B: %r" % (lb[i:i + 3],))
            if sorted(la) == sorted(lb):
                print("    (the same entries in another order in time: entries of concurrent streams share this queue id)")
    return same


def main():
    label, pa, pb = sys.argv[1:4]
    (ka, ca), (kb, cb) = load(pa), load(pb)
    nk = sum(len(q) for v in ka.values() for q in v)
    print("%s: A = %s, B = %s (%d kernels, %d queues)" % (label, pa, pb, nk, sum(len(v) for v in ka.values())))
    if nk == 0:
        print("  no kernels in run A: nothing was traced")
        return 1
    ok = compare("kernels", ka, kb)
    ok = compare("copies", ca, cb) and ok
    print("%s: %s" % (label, "SAME order of work" if ok else "DIFFERENT"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
