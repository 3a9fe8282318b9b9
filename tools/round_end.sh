#!/bin/bash
# tools/round_end.sh <tag> <outdir>: the round-end sequence on a GPU node - whole GPU suite, smoke, the --full bench line (with its
# detail record: the secondary workloads and the CPU baselines); writes <outdir>/<tag>_*
export TMPDIR=/tmp
R=${1:?usage: tools/round_end.sh <tag> <outdir>}
D=${2:?usage: tools/round_end.sh <tag> <outdir>}
mkdir -p "$D"
timeout 1500 python -m pytest tests -q -m gpu --durations=10 > "$D/${R}_gpu_tests.txt" 2>&1; tail -4 "$D/${R}_gpu_tests.txt"
python -c "import __graft_entry__ as g; g.smoke()" > "$D/${R}_smoke.txt" 2>&1; tail -1 "$D/${R}_smoke.txt"
( time timeout 1200 python bench.py --gpus 1 --steps 20 --warmup 5 --full ) > "$D/${R}_bench_stdout.txt" 2> "$D/${R}_bench_stderr.txt"
tail -1 "$D/${R}_bench_stdout.txt" > "$D/${R}_bench_line.json"; cp bench_detail.json "$D/${R}_bench_detail.json"
tail -4 "$D/${R}_bench_stderr.txt"; python - "$D/${R}_bench_line.json" <<P
import json, sys
j=json.load(open(sys.argv[1]))
print("value %.4g ms %.4f frac %.3f cpu %s" % (j["value"], j["ms_per_step"], j["roofline"]["frac"], j.get("cpu_baseline",{}).get("value")))
for s in j.get("secondary", []):
    print(s.get("key"), s.get("value"), s.get("frac"), s.get("mfma_busy"), s.get("kernel"), s.get("cpu"), s.get("extras"), s.get("error"))
print(len(json.dumps(j)))
P
