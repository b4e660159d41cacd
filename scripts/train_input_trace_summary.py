"""Kernel-time summary of loader-fed training steps in a `rocprofv3 --kernel-trace` database of
`scripts/bench_train_input.py --mode loader`: the time of the two train_input kernels per batch and their share of all kernel time.

    python scripts/train_input_trace_summary.py <rocprofv3 output directory>
"""
import collections
import glob
import json
import sqlite3
import sys

db = glob.glob(sys.argv[1] + "/**/*.db", recursive=True)[0]
rows = sqlite3.connect(db).execute("select name, duration from kernels order by start").fetchall()
short = lambda n: n.split("(")[0].replace("void ", "")
per, cnt = collections.Counter(), collections.Counter()
for n, d in rows:
    per[short(n)] += d
    cnt[short(n)] += 1
tot = sum(per.values())
new = {k: per[k] for k in ("train_input_h_kernel", "train_input_v_kernel")}
batches = cnt["train_input_v_kernel"]
out = {"batches_traced": batches, "kernel_time_ms_per_batch": round(tot / batches / 1e6, 3),
       "train_input_us_per_batch": {k: round(v / batches / 1e3, 1) for k, v in new.items()},
       "train_input_share_of_kernel_time": round(sum(new.values()) / tot, 5)}
print(json.dumps(out))
print("kernel,calls,total_us,share")
for k, v in per.most_common(12):
    print("%s,%d,%.1f,%.5f" % (k, cnt[k], v / 1e3, v / tot))
