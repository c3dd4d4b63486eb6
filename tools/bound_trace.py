#!/usr/bin/env python3
"""The bound path's launch groups in a rocprofv3 kernel trace
(*_kernel_trace.csv of a bench.py run): the dispatches of the largest burst
(gaps > --split us separate bursts: the timed call) are cut per stream into
groups from k_generate to k_bound_select; prints the mean dispatch of every
launch of a group (the scoring launches named by the list they score: before
k_bound_contenders the seeds, after it the contenders), a group's first start
to last end, and the burst's span per group.
usage: bound_trace.py TRACE.csv [--split 200]"""
import argparse
import collections
import csv
import re
import statistics

ap = argparse.ArgumentParser()
ap.add_argument("trace")
ap.add_argument("--split", type=float, default=200.0)
a = ap.parse_args()
rows = []
for r in csv.DictReader(open(a.trace)):
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("gcr::", "")
    name = re.sub(r"^void\s+|\(.*$", "", name)
    q = r.get("Stream_Id") or r.get("Queue_Id") or "0"
    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), q, name))
rows.sort()
bursts, cur, last_end = [], [], 0
for row in rows:
    if cur and (row[0] - last_end) / 1e3 > a.split:
        bursts.append(cur)
        cur = []
    cur.append(row)
    last_end = max(last_end, row[1]) if len(cur) > 1 else row[1]
bursts.append(cur)
burst = max(bursts, key=len)
per_q = collections.defaultdict(list)
for row in burst:
    per_q[row[2]].append(row)
groups = []
for q, rs in per_q.items():
    g = None
    for s, e, _, name in rs:
        if name.startswith("k_generate"):
            g = []
        if g is None:
            continue
        g.append((s, e, name))
        if name.startswith("k_bound_select"):
            groups.append(g)
            g = None
print(f"{len(rows)} dispatches, {len(bursts)} bursts; the largest: {len(burst)} dispatches on {len(per_q)} streams, "
      f"{len(groups)} groups")
if not groups:
    raise SystemExit("no k_generate .. k_bound_select group in the burst")
dur = collections.defaultdict(list)
for g in groups:
    after = False
    for s, e, name in g:
        if name.startswith("k_bound_contenders"):
            after = True
        scoring = name.startswith("k_score_split") or name.startswith("k_list_")
        label = f"{name} [{'contenders' if after else 'seeds'}]" if scoring else name
        dur[label].append((e - s) / 1e3)
tot = sum(sum(v) for v in dur.values())
for label, v in dur.items():
    print(f"  {label:60s} {len(v) / len(groups):5.2f} a group  mean {statistics.mean(v):8.1f} us  "
          f"median {statistics.median(v):8.1f} us  {100.0 * sum(v) / tot:5.1f} % of the kernel time")
chain = [(g[-1][1] - g[0][0]) / 1e3 for g in groups]
span = (max(r[1] for r in burst) - burst[0][0]) / 1e3
print(f"  a group, first start to last end: mean {statistics.mean(chain):.1f} us  median {statistics.median(chain):.1f} us")
print(f"  burst span {span:.1f} us, span per group {span / len(groups):.1f} us, "
      f"kernel time in flight {tot / span:.2f}")
