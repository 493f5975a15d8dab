"""The radix schedules and the tail rounds of sumcheck_host.hpp without a GPU: radix_run (one table, and sharded by rows over ranks
that are threads), radix_run_batch and SumcheckRounds::tail_rounds over plain C++ data passes in a stand-alone driver
(tests/c_driver/radix_host.cpp), built with AddressSanitizer + UndefinedBehaviorSanitizer -- and once more with ThreadSanitizer for
the sharded runs -- and run as a child process.  Every proof is compared word for word with the oracle's prover."""
import os
import subprocess

import numpy as np
import pytest

import exact_ref
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
SENTINEL = 0xA5A5A5A5A5A5A5A5
OK, NOT_CANONICAL, HIP, COMM = 0, 102, 101, 105
ORACLE_MAX = 1 << 13  # longer tables: the vectorised exact reference


def _build(tmp_path_factory, name, sanitize):
    exe = str(tmp_path_factory.mktemp(name) / "radix_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + sanitize +
                          ["-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "c_driver", "radix_host.cpp")] + srcs + ["-o", exe])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory, "radix", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def _run(exe, tmp_path, commands):
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(commands) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout.split("\n")[:-1]


def _words(line):
    head, rounds, point, fe = line.split(":")
    return head.split(), [int(x) for x in rounds.split()], [int(x) for x in point.split()], int(fe)


def _table(seed, n):
    if seed == 1:
        return np.full(n, P - 1, dtype=np.uint64)
    if seed == 2:
        return np.concatenate([np.zeros(n // 2, dtype=np.uint64), np.full(n // 2, P - 1, dtype=np.uint64)])
    return O.splitmix64_field(seed, n)


_refs = {}


def _reference(seed, n, fixed_seed=0):
    key = (seed, n, fixed_seed)
    if key not in _refs:
        t = _table(seed, n)
        ch = O.splitmix64_field(fixed_seed, n.bit_length() - 1) if fixed_seed else None
        r, p, fe = O.sumcheck_prove(P, t, ch) if n <= ORACLE_MAX else exact_ref.sumcheck_prove(t, ch)
        _refs[key] = ([int(x) for x in r], [int(x) for x in p], int(fe))
    return _refs[key]


def _run_cmd(world, n_local, seed, fixed_seed=0, bad_round=-1, sums_global=0, fail_rank=-1, fail_op=0):
    return "run %d %d %d %d %d %d %d %d" % (world, n_local, seed, fixed_seed, bad_round, sums_global, fail_rank, fail_op)


def test_single_table_proofs_equal_the_oracle(driver, tmp_path):
    """tail only (2, 1024), the first staged size (2048: k = 3), k = 10 then the tail (2^18), k = 10 then one more stage (2^19);
    Fiat-Shamir and fixed challenges; random tables and the two extreme patterns"""
    cases = [(n, seed, fs) for n in (2, 1024, 2048, 1 << 18, 1 << 19) for seed, fs in ((9100 + n % 97, 0), (9100 + n % 97, 9200))]
    cases += [(n, seed, 0) for n in (1024, 2048) for seed in (1, 2)]
    lines = _run(driver, tmp_path, [_run_cmd(1, n, seed, fs) for n, seed, fs in cases])
    assert len(lines) == len(cases)
    for (n, seed, fs), line in zip(cases, lines):
        head, rounds, point, fe = _words(line)
        assert head == ["run", "0", str(OK), "0", "0"], (n, seed, fs, head)
        assert (rounds, point, fe) == _reference(seed, n, fs), (n, seed, fs)


SHARDED = [(world, n_local, g) for world in (2, 4) for n_local in (1, 512, 4096) for g in (0, 1)]


def _check_sharded(lines):
    at = 0
    for world, n_local, g in SHARDED:
        ref = _reference(9300 + n_local, world * n_local)
        calls = set()
        for rank in range(world):
            head, rounds, point, fe = _words(lines[at + rank])
            assert head[:4] == ["run", str(rank), str(OK), "0"], (world, n_local, g, head)
            assert (rounds, point, fe) == ref, (world, n_local, g, rank)
            calls.add(head[4])
        # one exchange per stage unless the passes reduce themselves, and one for the tail
        stages = 1 if n_local > 1024 else 0
        assert calls == {str((0 if g else stages) + 1)}, (world, n_local, g, calls)
        at += world
    assert at == len(lines)


def test_sharded_proofs_equal_the_single_table_proof(driver, tmp_path):
    """ranks as threads, the all-gather a barrier over a shared buffer: every rank prints the proof of the interleaved table,
    without and with sums_global (the stand-in passes then add over the ranks themselves)"""
    _check_sharded(_run(driver, tmp_path, [_run_cmd(w, nl, 9300 + nl, sums_global=g) for w, nl, g in SHARDED]))


def test_sharded_runs_under_thread_sanitizer(tmp_path_factory, tmp_path):
    exe = _build(tmp_path_factory, "radix_tsan", ["-fsanitize=thread"])
    _check_sharded(_run(exe, tmp_path, [_run_cmd(w, nl, 9300 + nl, sums_global=g) for w, nl, g in SHARDED]))


@pytest.mark.parametrize("world", [2, 4])
def test_a_failing_pass_ends_every_rank_at_the_same_exchange(driver, tmp_path, world):
    """the rank whose fold (local length 4096) or read_tail (512) fails returns its own status, the others ZIGZ_ERR_COMM with the
    text for the context, after the same number of all-gathers; nobody writes a final_eval"""
    bad = world - 1
    cases = [(4096, 1, 2), (512, 2, 1)]  # local length, failing pass, all-gathers: block sums + tail; tail
    lines = _run(driver, tmp_path, [_run_cmd(world, nl, 9400, fail_rank=bad, fail_op=op) for nl, op, _ in cases])
    assert len(lines) == world * len(cases)
    for c, (nl, op, gathers) in enumerate(cases):
        for rank in range(world):
            head, rounds, point, fe = _words(lines[c * world + rank])
            exp = [str(HIP), "0"] if rank == bad else [str(COMM), "2"]
            assert head == ["run", str(rank)] + exp + [str(gathers)], (nl, op, head)
            assert fe == SENTINEL


def test_batch_tables_equal_their_own_runs(driver, tmp_path):
    """k = 1 and k = 5 with a repeated size: each table's words are those of its own radix_run and of the oracle; a pass error is
    returned as it is"""
    five = [(2, 9501), (1024, 9502), (2048, 9503), (1 << 13, 9504), (2048, 9505)]
    cmds = ["batch 0 0 1 2048 9500"]
    cmds += ["batch %d 0 5 " % fs + " ".join("%d %d" % x for x in five) for fs in (0, 9600)]
    cmds += [_run_cmd(1, n, seed) for n, seed in five]
    cmds += ["batch 0 1 5 " + " ".join("%d %d" % x for x in five)]
    lines = _run(driver, tmp_path, cmds)
    assert len(lines) == 2 + 6 + 6 + 5 + 6
    assert lines[0] == "batch %d" % OK and _words(lines[1])[1:] == _reference(9500, 2048)
    assert lines[2] == lines[8] == "batch %d" % OK
    own = [_words(x) for x in lines[14:19]]
    chs = O.splitmix64_field(9600, sum(n.bit_length() - 1 for n, _ in five))
    voff = 0
    for i, (n, seed) in enumerate(five):
        assert own[i][0][:3] == ["run", "0", str(OK)]
        assert _words(lines[3 + i])[0] == ["table", str(i)]
        assert _words(lines[3 + i])[1:] == own[i][1:] == _reference(seed, n), i
        v = n.bit_length() - 1
        r, p, fe = O.sumcheck_prove(P, _table(seed, n), chs[voff: voff + v])
        assert _words(lines[9 + i])[1:] == ([int(x) for x in r], [int(x) for x in p], int(fe)), i
        voff += v
    assert lines[19] == "batch %d" % HIP
    for i, line in enumerate(lines[20:]):  # the first stage's rounds were written, no final_eval
        assert _words(line)[3] == SENTINEL, i


@pytest.mark.parametrize("bad_round", [0, 1, 6])
def test_a_fixed_challenge_of_p_fails_lazily(driver, tmp_path, bad_round):
    """n = 2048 (a stage of 3 rounds, 8 rounds in the tail): a fixed challenge equal to p at round 0, in the middle of the stage
    and in the tail is ZIGZ_ERR_NOT_CANONICAL after that round's coefficients are recorded and before its point word is"""
    n, nv = 2048, 11
    head, rounds, point, fe = _words(_run(driver, tmp_path, [_run_cmd(1, n, 9700, 9701, bad_round)])[0])
    assert head == ["run", "0", str(NOT_CANONICAL), "0", "0"]
    ch = O.splitmix64_field(9701, nv)
    ch[bad_round] = 0  # (any canonical value: the words through this round do not depend on it)
    r, p, _ = O.sumcheck_prove(P, _table(9700, n), ch)
    w = 2 * (bad_round + 1)
    assert rounds[:w] == [int(x) for x in r[:w]] and rounds[w:] == [SENTINEL] * (2 * nv - w)
    assert point[:bad_round] == [int(x) for x in p[:bad_round]] and point[bad_round:] == [SENTINEL] * (nv - bad_round)
    assert fe == SENTINEL


def test_tail_rounds_at_one_factor_are_the_linear_tail(driver, tmp_path):
    """all p - 1, and low half 0 with high half p - 1 (every sum and difference at its extreme), at 1024 and below"""
    cases = [(n, seed) for n in (2, 64, 1024) for seed in (1, 2, 9800)]
    lines = _run(driver, tmp_path, ["tail %d %d" % c for c in cases])
    assert len(lines) == 2 * len(cases)
    for i, (n, seed) in enumerate(cases):
        new, old = _words(lines[2 * i]), _words(lines[2 * i + 1])
        assert new[0] == old[0] == ["tail", str(OK)]
        assert new[1:] == old[1:] == _reference(seed, n), (n, seed)
