#!/bin/bash
out=gpurun_out/r4d; mkdir -p $out
run() { name=$1; shift; timeout -k 10 400 python bench.py --full --no-extras --no-cpu-baseline "$@" > $out/$name.json 2> $out/$name.err || echo "$name failed"; python - <<PY
import json
try:
    d=json.load(open("$out/$name.json"))
    ph=d["detail"]["host_phase_ms_per_proof"]
    print("$name", "value %.0f M" % (d["value"]/1e6), "lanes", d["config"]["traces_per_step_per_gpu"], "slots", d["config"]["gpu_slots"], "cpu/proof %.2f" % d["detail"]["host_cpu_ms_per_proof"], "busy %.1f" % d["detail"]["host_cpus_busy"], {k: round(v,2) for k,v in ph.items() if v>0.05}, "frac %.3f busy %.2f" % (d["roofline"]["frac"], d["roofline"].get("busy_share_of_wall") or 0))
except Exception as e:
    print("$name", "no line", e)
PY
}
run nv16_b16 --nv 16 --slots 6
ZIGZ_BENCH_BATCH_MAX=8 run nv16_b8 --nv 16 --slots 8
ZIGZ_BENCH_BATCH_MAX=32 ZIGZ_BENCH_BATCH_LINGER_US=400 run nv16_b32 --nv 16 --slots 4
ZIGZ_BENCH_BATCH_MAX=16 run nv16_b16_l160 --nv 16 --slots 6 --batch 160
ZIGZ_BENCH_NO_BATCHING=1 run nv16_nobatch --nv 16 --slots 48
run nv12_b16 --nv 12 --slots 6
run nv17_b16 --nv 17 --slots 6
run nv20_s12 --slots 12
run nv24 --nv 24 --steps 3 --warmup 1
