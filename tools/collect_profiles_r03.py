#!/usr/bin/env python3
"""python tools/collect_profiles_r03.py OUTDIR: copies what tools/regen_profiles_r03.sh left in OUTDIR as p3_* into profiles/
(r03_ names) and derives, per kernel of ONE lone 2^20 proof, launches / time / HBM traffic / VALU instructions (profiles/r03_one_proof_kernels.json) and the traffic record
bench.py reads for `roofline.traffic` (profiles/r03_traffic.json).  Run from the repo root with the profile run's
OUTDIR at hand."""
import collections
import csv
import glob
import json
import os
import re
import shutil
import sys

ROUND = "r03"

def newest(pattern):
    files = glob.glob(pattern, recursive=True)
    assert files, pattern
    return max(files, key=os.path.getmtime)


def short(n):
    return re.sub(r"\(.*", "", n).replace("void ", "").replace("zk::", "")


def counters(path, names):
    """per dispatch (in dispatch order): (kernel, {counter: value})"""
    rows = collections.OrderedDict()
    for r in csv.DictReader(open(path)):
        if r["Counter_Name"] in names:
            key = int(r["Dispatch_Id"])
            rows.setdefault(key, (short(r["Kernel_Name"]), {}))[1][r["Counter_Name"]] = float(r["Counter_Value"])
    return [rows[k] for k in sorted(rows)]


def last_build(disp):
    """the dispatches of the last Merkle build in the file (tools/trace_one_proof.py proves three times)"""
    starts = [i for i, (k, _) in enumerate(disp) if k.startswith("k_runs_stage<true>")]
    i0 = starts[-1]
    out = []
    for k, c in disp[i0:]:
        out.append((k, c))
        if k.startswith("k_job_summary"):
            break
    return out


def main():
    one = newest(SRC + "/p3_one/**/*kernel_trace.csv")
    rows = sorted(csv.DictReader(open(one)), key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "k_runs_stage<true>" in r["Kernel_Name"]]
    build = []
    for r in rows[starts[-1]:]:
        build.append(r)
        if "k_job_summary" in r["Kernel_Name"]:
            break
    t0 = int(build[0]["Start_Timestamp"])
    with open("profiles/%s_one_proof_launches.csv" % ROUND, "w") as f:
        f.write("kernel,workitems,start_us,duration_us\n")
        for r in build:
            f.write("%s,%s,%.1f,%.1f\n" % (short(r["Kernel_Name"]), r.get("Grid_Size", r.get("Grid_Size_X", "")),
                                         (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    dur = collections.defaultdict(lambda: [0, 0.0])
    for r in build:
        d = dur[short(r["Kernel_Name"])]
        d[0] += 1
        d[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    F = last_build(counters(newest(SRC + "/p3_one_FETCH/**/*counter_collection.csv"), {"FETCH_SIZE"}))
    W = last_build(counters(newest(SRC + "/p3_one_WRITE/**/*counter_collection.csv"), {"WRITE_SIZE"}))
    V = last_build(counters(newest(SRC + "/p3_one_VALU/**/*counter_collection.csv"), {"SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU2"}))
    per = collections.defaultdict(lambda: {"launches": 0, "us": 0.0, "fetch_bytes": 0.0, "write_bytes": 0.0, "valu_wave_instr": 0.0,
                                           "valu2_wave_instr": 0.0})
    for k, (n, us) in dur.items():
        per[k]["launches"], per[k]["us"] = n, us
    for k, c in F:  # FETCH_SIZE is in KB and, on gfx950, counts half of the bytes of wide coalesced reads (MI355X_MICROARCH.md)
        per[k]["fetch_bytes"] += c.get("FETCH_SIZE", 0.0) * 2048
    for k, c in W:
        per[k]["write_bytes"] += c.get("WRITE_SIZE", 0.0) * 1024
    for k, c in V:
        per[k]["valu_wave_instr"] += c.get("SQ_INSTS_VALU", 0.0)
        per[k]["valu2_wave_instr"] += c.get("SQ_ACTIVE_INST_VALU2", 0.0)
    # what the hashing kernels hashed in that proof: the bench trace at 2^20 (stats of the same build through the API)
    stats_path = SRC + "/p3_one_stats.json"
    st = json.load(open(stats_path)) if os.path.exists(stats_path) else {}
    hashes = {"k_level_hash": st.get("list_hash_perms")}
    N = 1 << 20
    alg = {  # algorithmic HBM bytes of one lone proof's launches, per kernel family
        "k_level_hash": None if not hashes["k_level_hash"] else 96.0 * hashes["k_level_hash"],  # 64 B of children in, 32 B out
        "k_runs_stage<true>": 4.0 * 33 * N,                       # the 33 run-aware columns, read once
        "k_cons_leaf_insert": 4.0 * 10 * N,                       # the group's 10 columns, read once per pass
        "k_cons_pass<true>": 4.0 * 10 * N + 4.0 * N,              # ... and once more + one slot per leaf written
        "k_cons_pass<false>": 12.0 * N,                           # levels 1..12: 8 B of children's slots in, 4 B out per node
        "k_radix_fold<true>": 43 * (4.0 * N + 16 * 1024 * 8),
    }
    out = {}
    fam = collections.defaultdict(lambda: {"launches": 0, "us": 0.0, "hbm_bytes": 0.0, "valu_wave_instr": 0.0, "valu2_wave_instr": 0.0})
    for k, v in per.items():
        f = "k_level_hash" if k.startswith("k_level_hash") else k
        fam[f]["launches"] += v["launches"]
        fam[f]["us"] += v["us"]
        fam[f]["hbm_bytes"] += v["fetch_bytes"] + v["write_bytes"]
        fam[f]["valu_wave_instr"] += v["valu_wave_instr"]
        fam[f]["valu2_wave_instr"] += v["valu2_wave_instr"]
    for f, v in sorted(fam.items(), key=lambda kv: -kv[1]["us"]):
        rec = dict(v)
        if alg.get(f):
            rec["algorithmic_bytes"] = alg[f]
            rec["traffic_ratio"] = v["hbm_bytes"] / alg[f]
        if v["valu_wave_instr"]:
            rec["valu2_share"] = v["valu2_wave_instr"] / v["valu_wave_instr"]
        if f == "k_level_hash" and hashes[f]:
            rec["hashes"] = hashes[f]
            rec["hbm_bytes_per_hash"] = v["hbm_bytes"] / hashes[f]
            rec["valu_lane_instr_per_hash"] = v["valu_wave_instr"] * 64 / hashes[f]
            rec["gperm_per_s"] = hashes[f] / 1e9 / (v["us"] / 1e6)
        out[f] = rec
    src = ("rocprofv3 --kernel-trace / --pmc FETCH_SIZE / --pmc WRITE_SIZE / --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU2 (separate passes) "
           "-- python3 tools/trace_one_proof.py: the launches of ONE lone 2^20 proof of the bench trace; FETCH_SIZE doubled per "
           "MI355X_MICROARCH.md (gfx950 reports 1/2 of wide coalesced reads), KB -> bytes x1024")
    json.dump({"source": src, "kernels": out}, open("profiles/%s_one_proof_kernels.json" % ROUND, "w"), indent=1)
    if "k_level_hash" in out and "hbm_bytes_per_hash" in out["k_level_hash"]:
        r = out["k_level_hash"]
        json.dump({"source": "profiles/%s_one_proof_kernels.json" % ROUND,
                   "k_level_hash": {"hbm_bytes_per_hash": r["hbm_bytes_per_hash"], "algorithmic_bytes_per_hash": 96.0,
                                    "valu_lane_instr_per_hash": r.get("valu_lane_instr_per_hash"), "valu2_share": r.get("valu2_share"),
                                    "hashes_in_the_profiled_proof": r["hashes"]}},
                  open("profiles/%s_traffic.json" % ROUND, "w"), indent=1)
    for f, r in out.items():
        print("%-26s launches %3d  %8.1f us  %9.2f MB HBM%s%s" % (
            f, r["launches"], r["us"], r["hbm_bytes"] / 1e6,
            ("  (%.2f x algorithmic)" % r["traffic_ratio"]) if "traffic_ratio" in r else "",
            ("  valu2 %.2f" % r["valu2_share"]) if "valu2_share" in r else ""))
    shutil.copy(newest(SRC + "/p3_one_FETCH/**/*counter_collection.csv"), "profiles/%s_pmc_fetch_size.csv" % ROUND)
    shutil.copy(newest(SRC + "/p3_one_WRITE/**/*counter_collection.csv"), "profiles/%s_pmc_write_size.csv" % ROUND)
    shutil.copy(newest(SRC + "/p3_one_VALU/**/*counter_collection.csv"), "profiles/%s_pmc_valu.csv" % ROUND)
    for tag in ("kernels", "b1", "bdef", "lasso", "sumcheck"):
        shutil.copy(newest(SRC + "/p3_%s/**/*kernel_stats.csv" % tag), "profiles/%s_%s_kernel_stats.csv" % (ROUND, tag))
    for src_, dst in (("p3_kernels.json", "kernels.json"), ("p3_kernels_plain.json", "kernels_unprofiled.json"),
                      ("p3_bench.json", "final_bench.json"), ("p3_bench_b1.json", "final_bench_b1.json"),
                      ("p3_bench_8x8.json", "final_bench_8x8.json"), ("p3_bench_11x8.json", "final_bench_11x8.json"),
                      ("p3_bench_s0.json", "final_bench_own_thread_transcripts.json"), ("p3_gpu_bound.txt", "gpu_bound_rate.txt"),
                      ("p3_lasso.json", "lasso.json"), ("p3_sumcheck.json", "sumcheck.json"), ("p3_extra.json", "extra.json"),
                      ("p3_configs.jsonl", "configs.jsonl")):
        if os.path.exists(os.path.join(SRC, src_)):
            shutil.copy(os.path.join(SRC, src_), "profiles/%s_%s" % (ROUND, dst))
    for name in ("final_bench", "final_bench_b1", "final_bench_8x8", "final_bench_11x8", "final_bench_own_thread_transcripts"):
        pth = "profiles/%s_%s.json" % (ROUND, name)
        if not os.path.exists(pth):
            continue
        d = json.loads(open(pth).read().strip().splitlines()[-1])
        r = d["roofline"]
        print("%-36s %7.1f M steps/s  %.3f ms/proof  %s frac %.3f  in-proof %s  bind %s" %
              (name, d["value"] / 1e6, d["config"]["ms_per_proof_per_gpu"], r["kernel"], r["frac"], r.get("in_proof_frac"),
               r.get("bind_hbm_frac")))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: python %s OUTDIR  (the directory the profile run wrote)" % sys.argv[0])
    SRC = sys.argv[1]
    main()
