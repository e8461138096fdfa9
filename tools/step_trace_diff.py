#!/usr/bin/env python
"""Compares two rocprofv3 csv traces of tools/step_trace.py or of tools/rank_trace.py (--hip-runtime-trace --kernel-trace -f csv):

  * the sequence of HIP API call names on the thread that made the most calls (the one that drives the engine), and
  * the sequence of kernel names per queue (and per stream, where the trace names streams), in dispatch order, with the queue /
    stream handles renamed by order of first appearance.

The API sequence holds the calls' NAMES only, not their arguments: a wait or a record that moved to another stream under the same name
shows here only through the kernel order per queue / stream. "identical" means no more than that.

Prints the lengths and the first differences; exits 1 when a sequence differs.   tools/step_trace_diff.py <dir 1> <dir 2>"""
import csv
import difflib
import glob
import os
import sys
from collections import Counter, OrderedDict


def rows(directory, suffix):
    files = sorted(glob.glob(os.path.join(directory, "**", "*" + suffix), recursive=True))
    if len(files) != 1:
        sys.exit("expected one *%s under %s, found %d" % (suffix, directory, len(files)))
    with open(files[0], newline="") as f:
        return list(csv.DictReader(f))


def api_sequence(directory):
    r = rows(directory, "hip_api_trace.csv")
    thread = Counter(x["Thread_Id"] for x in r).most_common(1)[0][0]
    r = [x for x in r if x["Thread_Id"] == thread]
    r.sort(key=lambda x: int(x["Start_Timestamp"]))
    return [x["Function"] for x in r]


def kernel_sequences(directory, column):
    r = rows(directory, "kernel_trace.csv")
    if not r:
        sys.exit("the kernel trace under %s is empty" % directory)
    if column not in r[0]:
        return None
    r.sort(key=lambda x: int(x["Dispatch_Id"]))
    out = OrderedDict()
    for x in r:
        out.setdefault(x[column], []).append(x["Kernel_Name"])
    return ["%s %d: %s" % (column, i, name) for i, names in enumerate(out.values()) for name in names]


def compare(what, a, b):
    if a == b:
        print("%s: identical, %d entries" % (what, len(a)))
        return True
    print("%s: DIFFERENT, %d against %d entries" % (what, len(a), len(b)))
    for line in list(difflib.unified_diff(a, b, "first", "second", n=3, lineterm=""))[:80]:
        print("    " + line)
    return False


def main():
    d1, d2 = sys.argv[1:3]
    ok = compare("HIP API calls of the calling thread", api_sequence(d1), api_sequence(d2))
    for column in ("Queue_Id", "Stream_Id"):
        a, b = kernel_sequences(d1, column), kernel_sequences(d2, column)
        if a is None or b is None:
            print("kernels per %s: the trace has no such column" % column)
            continue
        ok = compare("kernels per %s" % column, a, b) and ok
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
