#!/bin/bash
# tools/run_gpu_batch.sh <output dir> — the closing check on an MI355X box, from the repo root: the GPU tests, the full bench
# line, smoke(); the logs and the bench line go into <output dir>.
set -u
OUT=${1:?usage: tools/run_gpu_batch.sh <output dir>}
mkdir -p "$OUT"
MX_FAULT_LOG="$OUT/fault_sweep_r06_device.log" MX_RCCL_LOG="$OUT/rccl_r06.log" timeout 2400 python -m pytest tests -m gpu -q 2>&1 | tail -5
python bench.py --full > "$OUT/bench_check.json" 2> "$OUT/bench_check.err"
OUT="$OUT" python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "bench_check.json")))
pv = d["phase_vocoder_supplementary"]
print({k: d[k] for k in ("value", "ms_per_step", "outputs_ok", "library_src_sha")}, d["roofline"]["frac"], d["roofline"]["traffic"], pv["call_ms"], pv["arena_bytes"], pv["chunks"], d.get("gpu_over_cpu_step"))
PY
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" 2>&1 | tail -1
