# One GPU run at the end of a round: the GPU test suite, smoke(), the full bench line (--full), and the rocprofv3 kernel trace of a
# lean bench run (summaries are copied into profiles/ by hand afterwards).  usage: bash scripts/round_end_run.sh OUT_DIR
out=$(mkdir -p "${1:?usage: bash scripts/round_end_run.sh OUT_DIR}" && cd "$1" && pwd)
repo=$(cd "$(dirname "$0")/.." && pwd)
cd "$repo"
timeout 1200 python -m pytest tests -m gpu -q 2>&1 | tail -8 > $out/pytest.txt
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $out/smoke.txt 2>&1
timeout 600 python bench.py --full > $out/bench.json 2> $out/bench.err
cd /tmp && export TMPDIR=/tmp && timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/prof -o bench -- python $repo/bench.py --steps 20 --warmup 5 > $out/bench_prof.json 2>/dev/null
cd "$repo"; tail -3 $out/pytest.txt; tail -2 $out/smoke.txt; python - "$out/bench.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
r = d["roofline"]
print("value", d["value"], d["ms_per_step"], "batched", d["value_inference_batched"]["value"], "pipelined", d["pipelined"]["value"], "graphed", (d.get("graphed") or {}).get("value"))
print({k: r.get(k) for k in ("frac", "achieved", "traffic", "backbone_mfma_busy", "step_traffic", "step_traffic_over_algorithmic")})
print("parity", d["timed_batch_parity"]["gate"], d["timed_batch_parity"]["deviation_among_matched"]["box_median"], d["timed_batch_parity"]["bars"]["box_median"])
print("knn", d["knn"].get("ms_per_sweep"), {k: v.get("ms") for k, v in d["bandwidth_kernels"].items() if isinstance(v, dict)})
print("cpu", d["cpu_baseline"]["value"])
PY
