"""bench.py --dump-outputs: the proofs of the timed region's last step as exact float32 / float64 arrays (every lane's SHA-256
and length, a seeded byte sample per lane within a size limit); on the GPU, `--steps` sets the timed steps, the line carries
ms_per_step, and the dumped proofs are those of Prover.prove on the same programs, whatever the lane count."""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def _check_dump(b, d, proofs, sampled, prefix=""):
    sha = np.load(os.path.join(d, prefix + "proof_sha256.npy"))
    ln = np.load(os.path.join(d, prefix + "proof_length.npy"))
    assert sha.dtype == np.float32 and sha.shape == (len(proofs), 32) and ln.dtype == np.float64
    for k, p in enumerate(proofs):
        assert sha[k].astype(np.uint8).tobytes() == hashlib.sha256(p).digest() and ln[k] == len(p)
    names = sorted(f for f in os.listdir(d) if f.startswith(prefix + "proof_lane"))
    assert names == ["%sproof_lane%03d.npy" % (prefix, k) for k in range(sampled)]
    for k in range(sampled):
        a = np.load(os.path.join(d, names[k]))
        assert a.dtype == np.float32
        pos = b.sample_positions(len(proofs[k]))
        assert np.array_equal(a.astype(np.uint8), np.frombuffer(proofs[k], dtype=np.uint8)[pos])


def test_dump_outputs_samples_exact_bytes_within_the_limit(tmp_path):
    b = _bench_module()
    rng = np.random.default_rng(1)
    big = rng.integers(0, 256, 3 * b.DUMP_SAMPLE_BYTES, dtype=np.uint8).tobytes()
    proofs = [big, bytes(range(256)) * 4, big[:-1]]
    pos = b.sample_positions(len(big))
    assert len(pos) == b.DUMP_SAMPLE_BYTES and np.all(np.diff(pos) >= 0) and pos[-1] < len(big)
    assert np.array_equal(pos, b.sample_positions(len(big))) and np.array_equal(b.sample_positions(1024), np.arange(1024))
    arrays = [np.frombuffer(p, dtype=np.uint8) for p in proofs]
    fixed = 3 * 32 * 4 + 3 * 8
    # room for the first two lanes' samples only: the digests and lengths still cover all three
    assert b.dump_outputs(str(tmp_path / "d"), arrays, limit=fixed + 4 * (b.DUMP_SAMPLE_BYTES + 1024)) == 2
    _check_dump(b, str(tmp_path / "d"), proofs, 2)
    assert b.dump_outputs(str(tmp_path / "r"), arrays, prefix="rank1_") == 3
    _check_dump(b, str(tmp_path / "r"), proofs, 3, prefix="rank1_")


def _env():
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    return e


def test_bench_refuses_zero_steps_and_dump_with_other_legs(tmp_path):
    for extra in (["--steps", "0"], ["--dry-run", "--dump-outputs", str(tmp_path)]):
        out = subprocess.run([sys.executable, BENCH] + extra, env=_env(), capture_output=True, text=True, timeout=120)
        assert out.returncode == 2, (extra, out.stderr[-2000:])
    assert not os.listdir(tmp_path)


@pytest.mark.gpu
def test_bench_dump_outputs_end_to_end(tmp_path):
    import programs
    import zigz_amd
    from zigz_amd import host
    b = _bench_module()
    nv = 16
    runs = []
    for batch in (2, 3):
        d = tmp_path / ("b%d" % batch)
        out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--nv", str(nv), "--batch",
                              str(batch), "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(d)],
                             env=_env(), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        j = json.loads(out.stdout.strip().split("\n")[-1])
        assert j["steps"] == 3 and j["ms_per_step"] > 0
        assert j["config"]["traces_per_step_per_gpu"] == batch
        runs.append(str(d))
    ctx = zigz_amd.Context(0)
    try:  # lane k proves the k-th program of the bench trace: the dump holds Prover.prove's proofs of those programs
        proofs = [host.prove(ctx, programs.add_xor_loop(((1 << nv) - 3) // 4 - k), 0x1000, None, 2 << nv)[0] for k in range(3)]
    finally:
        ctx.close()
    _check_dump(b, runs[0], proofs[:2], 2)
    _check_dump(b, runs[1], proofs, 3)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_legs():
    """A plain run sets up, warms up, times its steps and prints the line -- no CPU baseline, no roofline leg, no leg after the
    timed region --; --full runs all of them again and puts their figures into the line."""
    base = [sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--nv", "16", "--batch", "2"]
    out = subprocess.run(base, env=_env(), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads(out.stdout.strip().split("\n")[-1])
    assert j["unit"] == "trace steps/s" and j["higher_is_better"] is True and j["dtype"] == "u32"
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["steps"] == 2 and j["warmup"] == 1
    assert j["config"]["traces_per_step_per_gpu"] == 2
    assert "roofline" not in j and "cpu_baseline" not in j and "self_check_ok" not in j["config"]
    assert "bench.py: leg " not in out.stderr and "cpu_baseline child" not in out.stderr
    out = subprocess.run(base + ["--full", "--cpu-sample-cols", "1"], env=_env(), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    j = json.loads(out.stdout.strip().split("\n")[-1])
    assert j["value"] > 0 and j["roofline"]["kernel"] == "k_level_hash" and j["roofline"]["launches"] > 0
    assert j["cpu_baseline"]["value"] > 0 and j["config"]["self_check_ok"] is True
    assert "leg_errors" not in j["detail"], j["detail"]["leg_errors"]
    for key in ("single_proof_ms", "pcie_inclusive_value", "gpu_bound_ms_per_proof", "register_worst_case_value",
                "config4_mixed_value", "straight_line_value", "dense_merkle_value", "value_nv22", "value_nv24"):
        assert j["config"][key] > 0, key
    assert j["detail"]["kernel_leg"]
