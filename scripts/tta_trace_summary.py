"""Kernel-time summary of the test-time augmentation calls in a `rocprofv3 --kernel-trace` database of scripts/bench_tta.py: each call is
the span from its tta_resize_h_kernel to its tta_gather_kernel (resize launches not followed by a call -- the floor's buffers -- and
the floor's own launches are left out).  Prints a JSON summary line, then per-kernel CSV.

    python scripts/tta_trace_summary.py <rocprofv3 output directory>
"""
import collections
import glob
import json
import sqlite3
import sys

db = glob.glob(sys.argv[1] + '/*.db')[0]
c = sqlite3.connect(db)
rows = c.execute("select name, duration from kernels order by start").fetchall()
short = lambda n: n.split('(')[0].replace('void ', '')
idx = [i for i, r in enumerate(rows) if short(r[0]) == 'tta_resize_h_kernel']
gat = [i for i, r in enumerate(rows) if short(r[0]) == 'tta_gather_kernel']
# each TTA call: its resize pair .. its gather; resize pairs not followed by a call (the floor's buffers) are skipped
calls = []
for g in gat:
    s = max(i for i in idx if i < g)
    calls.append((s, g))
per = collections.Counter(); cnt = collections.Counter()
for s, g in calls:
    for n, d in rows[s:g + 1]:
        per[short(n)] += d; cnt[short(n)] += 1
tot = sum(per.values())
new = {k: per[k] for k in ('tta_resize_h_kernel', 'tta_resize_v_kernel', 'tta_union_kernel', 'tta_gather_kernel')}
merge_nms = 0
for s, g in calls:
    u = max(i for i in range(s, g + 1) if short(rows[i][0]) == 'tta_union_kernel')
    merge_nms += sum(d for n, d in rows[u + 1:g] )
out = {"tta_calls_traced": len(calls), "tta_kernel_time_ms_per_call": round(tot / len(calls) / 1e6, 3),
       "new_kernels_us_per_call": {k: round(v / len(calls) / 1e3, 1) for k, v in new.items()},
       "new_kernels_share": round(sum(new.values()) / tot, 5),
       "merge_nms_us_per_call": round(merge_nms / len(calls) / 1e3, 1),
       "new_kernels_plus_merge_nms_share": round((sum(new.values()) + merge_nms) / tot, 5)}
print(json.dumps(out))
print("kernel,calls,total_us,share")
for k, v in per.most_common():
    print("%s,%d,%.1f,%.5f" % (k, cnt[k], v / 1e3, v / tot))
