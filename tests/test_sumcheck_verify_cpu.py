"""Batched sumcheck verification and batched MLE evaluation without a GPU: the host header (argument checks, round replay with
the library's own transcript) built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone driver
(tests/c_driver/sumcheck_verify_host.cpp) and run as a child process against the oracle's verifier; the four entries in the
header, the ctypes table, the Zig binding and the library; the gfx950 assembly of mle_batch.hip (no scratch, the hand-off counts
behind a barrier)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import sumcheck_verify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
ENTRIES = ["zigz_dev_mle_eval_batch", "zigz_mle_eval_batch", "zigz_dev_sumcheck_verify_batch", "zigz_sumcheck_verify_batch"]
OK, EMPTY, NOT_POW2, NO_VARIABLES, NOT_CANONICAL, INVALID = 0, 1, 2, 5, 102, 103


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("scv") / "sumcheck_verify_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_driver", "sumcheck_verify_host.cpp")] + srcs + ["-o", exe])
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


@pytest.fixture(scope="module")
def proofs():
    """[(table, kind, claimed, rounds, point, final_eval)]: seeded and constant tables of n = 2 .. 2^13, honest and tampered"""
    out = []
    for i, n in enumerate([2, 4, 8, 1 << 10, 1 << 13]):
        for t in (O.splitmix64_field(4100 + i, n), np.full(n, 1234567 + i, dtype=np.uint64)):
            rounds, point, fe = O.sumcheck_prove(P, t)
            for kind, c, r, q, f in R.tampered(O.mle_sum(P, t), rounds, point, fe):
                out.append((t, kind, c, r, q, f))
    return out


def test_replay_gives_the_oracles_verdicts(driver, proofs, tmp_path):
    path = tmp_path / "proofs.txt"
    with open(path, "w") as fh:
        for t, kind, c, r, q, f in proofs:
            fh.write(" ".join(str(int(x)) for x in [len(q), c, f, *r, *q]) + "\n")
    lines = _run(driver, "replay", str(path)).split("\n")[:-1]
    assert len(lines) == len(proofs)
    verdicts = []
    for line, (t, kind, c, r, q, f) in zip(lines, proofs):
        ok, expected = (int(x) for x in line.split())
        pt = [int(x) for x in q]
        assert (bool(ok), expected) == R.claim_chain(c, r, len(pt)), (len(t), kind)
        # the reference's order: the oracle at the point as given
        ev = O.mle_eval(P, t, pt)
        got = bool(ok and ev == expected and ev == f)
        assert got == O.sumcheck_verify(P, t, c, r, q, f), (len(t), kind)
        verdicts.append(got)
        # the reversed point is where the prover's final_eval lives: every honest proof accepts, every tampered one rejects
        ev_r = O.mle_eval(P, t, pt[::-1])
        if kind == "honest":
            assert ok and ev_r == expected == f, (len(t), kind)
        elif int(t[0]) != int(t[1]) or kind != "point":  # (a constant's extension is that constant at every point)
            assert not (ok and ev_r == expected and ev_r == f), (len(t), kind)
    # n = 2 (one variable: eval([r]) = c0 + c1 r identically) and the constant tables accept under the reference's order;
    # the honest seeded tables of two or more variables do not
    assert True in verdicts and False in verdicts
    honest = [v for v, pr in zip(verdicts, proofs) if pr[1] == "honest"]
    assert True in honest and False in honest


def test_argument_checker(driver):
    got = {}
    for line in _run(driver, "check").split("\n")[:-1]:
        name, st, bad = line.split()
        got[name] = (int(st), int(bad))
    expect = {}
    for s in ("host", "dev"):
        expect.update({
            f"eval_ok_{s}": (OK, -1), f"eval_k0_{s}": (OK, -1), f"eval_k4097_{s}": (INVALID, -1),
            f"verify_ok_{s}": (OK, -1), f"verify_reversed_ok_{s}": (OK, -1), f"verify_k0_{s}": (OK, -1),
            f"verify_k4097_{s}": (INVALID, -1), f"verify_flag2_{s}": (INVALID, -1), f"verify_no_rejected_{s}": (INVALID, -1),
            # the single entries' statuses: eval takes a table of one value, the prover does not
            f"eval_n0_{s}": (EMPTY, 1), f"eval_n1_{s}": (OK, -1), f"eval_n3_{s}": (NOT_POW2, 1),
            f"verify_n0_{s}": (EMPTY, 1), f"verify_n1_{s}": (NO_VARIABLES, 1), f"verify_n3_{s}": (NOT_POW2, 1),
            f"eval_point3_{s}": (NOT_CANONICAL, 3), f"verify_point3_{s}": (NOT_CANONICAL, 3),
            f"verify_round1_{s}": (NOT_CANONICAL, 1), f"eval_ignores_rounds_{s}": (OK, -1),
            f"verify_claimed2_{s}": (NOT_CANONICAL, 2), f"verify_final0_{s}": (NOT_CANONICAL, 0),
            f"verify_first_of_two_{s}": (NOT_CANONICAL, 1), f"verify_p_minus_1_{s}": (OK, -1),
        })
    expect.update({
        "eval_value2_host": (NOT_CANONICAL, 2), "verify_value2_host": (NOT_CANONICAL, 2), "eval_null3_host": (INVALID, 3),
        "eval_misaligned1_dev": (INVALID, 1), "verify_misaligned1_dev": (INVALID, 1),
        "eval_null0_dev": (INVALID, 0), "verify_null0_dev": (INVALID, 0),
    })
    assert got == expect, {k: (got.get(k), expect.get(k)) for k in set(got) | set(expect) if got.get(k) != expect.get(k)}


def test_entries_in_header_binding_ctypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "zig", "zigz_hip.zig")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert f'pub extern "c" fn {name}(' in zig, name
    assert re.search(r"#define ZIGZ_SUMCHECK_VERIFY_POINT_REVERSED 1u\b", hdr)
    assert "pub const SUMCHECK_VERIFY_POINT_REVERSED = 1;" in zig
    assert re.search(r"#define ZIGZ_ABI_VERSION 1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name in ENTRIES:
        assert name in _ffi.SIGNATURES
    for m in ("dev_mle_eval_batch", "mle_eval_batch", "dev_sumcheck_verify_batch", "sumcheck_verify_batch"):
        assert callable(getattr(hip.Context, m))
    assert hip.SUMCHECK_VERIFY_POINT_REVERSED == 1


def test_mle_batch_kernels_use_no_scratch_and_count_behind_a_barrier():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import isa_counts
    from test_isa_handoff import handoffs
    asm = isa_counts.assembly(sources=("mle_batch.hip",))
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    assert len(names) == 2 and len(sizes) == 2, names  # k_mle_batch_eval, k_mle_batch_finish
    assert all(int(s) == 0 for s in sizes), dict(zip(names, sizes))
    found = handoffs(asm)
    assert {k for k, _, _ in found} == {"k_mle_batch_finish"}, found
    assert all(barrier for _, _, barrier in found), found
    # the table is read with 16-byte non-temporal loads, eight per lane
    assert len(re.findall(r"_load_dwordx4 .* nt\b", asm)) >= 8
