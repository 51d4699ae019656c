#!/usr/bin/env python3
"""Hardware queues in a rocprofv3 --kernel-trace: per kernel name the distinct Queue_Id values and, per queue, the streams whose
kernels ran on it.  trace_queues.py TRACE_DIR [substring of the kernel name]"""
import collections, csv, glob, sys
f = glob.glob(sys.argv[1] + "/**/*kernel_trace.csv", recursive=True)[0]
want = sys.argv[2] if len(sys.argv) > 2 else ""
per = collections.defaultdict(lambda: collections.defaultdict(collections.Counter))
for row in csv.DictReader(open(f)):
    name = row["Kernel_Name"].replace("void ", "").split("(")[0][:48]
    if want in name:
        per[name][int(row["Queue_Id"])][row.get("Stream_Id", "?")] += 1
for name, queues in sorted(per.items()):
    ids = sorted(queues)
    print(f"{name}: kernels {sum(sum(c.values()) for c in queues.values())}, {len(ids)} distinct queue ids {ids}")
    for q in ids:
        print(f"  queue {q}: " + ", ".join(f"stream {s} x {n}" for s, n in sorted(queues[q].items())))
