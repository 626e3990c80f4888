#!/bin/bash
# tools/gpu_batch_r06_evidence.sh <output dir> — round 6, VERDICT item 2: configs[4] (N = 16384 / hop 512) and resynthesis
# evidence at HEAD, one box: rocprofv3 stats + PMC passes, then the bench line (cpu_baseline included) with roofline.traffic
# from that PMC set.  tools/profile_gpu.sh writes its own directory (OUT there); <output dir> takes the bench line and logs.
set -u
OUT=${1:?usage: tools/gpu_batch_r06_evidence.sh <output dir>}
mkdir -p "$OUT"
bash tools/profile_gpu.sh r06_16384x512 --fft 16384 --hop 512 > "$OUT/profile_r06_16384x512.log" 2>&1
cp gpurun_out/pmc_latest_r06_16384x512.json profiles/pmc_latest_16384x512.json
python bench.py --full --fft 16384 --hop 512 > "$OUT/bench_r06_c4_16384x512.json" 2> "$OUT/bench_r06_c4_16384x512.err"
PROF_RESYNTH=1 bash tools/profile_gpu.sh r06_resynth > "$OUT/profile_r06_resynth.log" 2>&1
OUT="$OUT" python - <<'PY'
import json, os
d = json.load(open(os.path.join(os.environ["OUT"], "bench_r06_c4_16384x512.json")))
print({k: d[k] for k in ("value", "ms_per_step", "outputs_ok", "library_src_sha")}, d["roofline"]["frac"], d["roofline"]["traffic"], d["cpu_baseline"]["value"])
PY
tail -12 gpurun_out/prof_r06_16384x512_summary.txt
tail -8 gpurun_out/prof_r06_resynth_summary.txt
rocm-smi --showpower --showclocks 2>/dev/null | head -20 > "$OUT/r06_evidence_smi.txt"
