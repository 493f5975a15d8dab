"""The batched product sumcheck prover without a GPU: the numpy reference (sumcheck_product_ref.py) against the oracle's linear
prover at d = 1 and against the verifier's checks at d = 2, 3; the two entries in the header, the ctypes table, the Zig binding
and the library; the host header (argument checks, coefficient assembly from kernel-style sums, tail rounds, transcript) built with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone driver (tests/c_driver/product_host.cpp) and run as a child
process against the reference; the gfx950 assembly of sumcheck_product.hip (no scratch, the hand-offs count behind a barrier).
The reference is also pinned where the GPU tests lean on it alone: at 2^14 and 2^16 through the vectorised exact eval, on every
edge input of test_gpu_sumcheck_product_exact.py at 2^11, and a count shows that those inputs reach the equality case of every
compare in field.hpp's add_mod, sub_mod and monty_reduce."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import sumcheck_product_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
ENTRIES = ["zigz_dev_sumcheck_prove_product_batch", "zigz_sumcheck_prove_product_batch"]
OK, EMPTY, NOT_POW2, NO_VARIABLES, NOT_CANONICAL, INVALID = 0, 1, 2, 5, 102, 103


def tables(seed, d, n):
    return [O.splitmix64_field(seed + 17 * j, n) for j in range(d)]


@pytest.mark.parametrize("v", [1, 2, 5, 11])
def test_reference_at_degree_one_is_the_oracles_prover(v):
    t = O.splitmix64_field(7000 + v, 1 << v)
    claimed, rounds, point, evals, fe = R.prove([t])
    r0, p0, fe0 = O.sumcheck_prove(P, t)
    assert np.array_equal(rounds, r0) and np.array_equal(point, p0) and fe == fe0 == int(evals[0])
    assert claimed == O.mle_sum(P, t)
    ch = O.splitmix64_field(7100 + v, v)
    claimed, rounds, point, evals, fe = R.prove([t], ch)
    r0, p0, fe0 = O.sumcheck_prove(P, t, ch)
    assert np.array_equal(rounds, r0) and np.array_equal(point, p0) and fe == fe0 == int(evals[0])
    assert claimed == O.mle_sum(P, t)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("v", [1, 2, 5, 11])
def test_reference_proofs_verify(d, v):
    fs = tables(7200 + 10 * v + d, d, 1 << v)
    proof = R.prove(fs)
    assert len(proof[1]) == (d + 1) * v and len(proof[2]) == v and len(proof[3]) == d
    # the sum itself, term by term
    prod = np.ones(1 << v, dtype=np.uint64)
    for f in fs:
        prod = (prod * f) % np.uint64(P)
    assert proof[0] == int(np.sum(prod, dtype=np.uint64)) % P
    R.check_proof(fs, proof)
    ch = O.splitmix64_field(7300 + v, v)
    R.check_proof(fs, R.prove(fs, ch), fiat_shamir=False)
    # a changed coefficient breaks the chain
    bad = proof[1].copy()
    bad[len(bad) // 2] = (int(bad[len(bad) // 2]) + 1) % P
    ok, expected, _ = R.claim_chain(proof[0], bad, v, d)
    assert not (ok and expected == proof[4])


def _sum_of_products(fs):
    prod = np.ones(len(fs[0]), dtype=np.uint64)
    for f in fs:
        prod = (prod * f) % np.uint64(P)
    return int(np.sum(prod, dtype=np.uint64)) % P


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("v", [14, 16])
def test_reference_proofs_verify_beyond_the_oracles_eval(d, v):
    """the verifier's view with exact_ref.eval in place of the C oracle's O(v 2^v) eval, and the claimed sum term by term"""
    fs = tables(7700 + 10 * v + d, d, 1 << v)
    proof = R.prove(fs)
    assert len(proof[1]) == (d + 1) * v and len(proof[2]) == v and len(proof[3]) == d
    assert proof[0] == _sum_of_products(fs)
    R.check_proof(fs, proof, mle_eval=R.exact_mle_eval)
    fixed = R.prove(fs, O.splitmix64_field(7800 + v, v))
    assert fixed[0] == proof[0]
    R.check_proof(fs, fixed, fiat_shamir=False, mle_eval=R.exact_mle_eval)


def test_eval_hook_agrees_with_the_oracles_eval():
    fs = tables(7900, 3, 1 << 9)
    proof = R.prove(fs)
    R.check_proof(fs, proof)
    R.check_proof(fs, proof, mle_eval=R.exact_mle_eval)
    pt = [int(x) for x in proof[2]][::-1]
    assert [R.exact_mle_eval(f, pt) for f in fs] == [O.mle_eval(P, f, pt) for f in fs] == [int(x) for x in proof[3]]
    with pytest.raises(AssertionError):  # the hook is what decides: a wrong eval fails the check
        R.check_proof(fs, proof, mle_eval=lambda f, q: (R.exact_mle_eval(f, q) + 1) % P)


def test_step_patterns():
    up, down = R.pattern("step_up", 4), R.pattern("step_down", 4)
    assert list(up) == [0] * 8 + [P - 1] * 8 and list(down) == [P - 1] * 8 + [0] * 8
    assert np.array_equal(R.pattern("ramp", 4), np.arange(16, dtype=np.uint64))
    assert list(R.edge_challenges("zero_pm1", 5)) == [0, P - 1, 0, P - 1, 0] and R.edge_challenges("fs", 5) is None
    assert len(R.edge_cases(11)) == 7 * 3 * 6


def _edge_tables(nv):
    return {n: R.pattern(n, nv) for n in R.edge_pattern_names()}


def test_edge_proofs_verify():
    """every edge input of the GPU test at 2^11: the reference's proof passes the verifier's checks (claim chain, factor evals at
    the reversed point, their product) and claims the sum of the products term by term"""
    nv = 11
    tabs = _edge_tables(nv)
    for names, cname in R.edge_cases(nv) + [(R.REDUCE_EDGE, "fs")]:
        fs = [tabs[n] for n in names]
        proof = R.prove(fs, R.edge_challenges(cname, nv))
        assert proof[0] == _sum_of_products(fs), (names, cname)
        R.check_proof(fs, proof, fiat_shamir=cname == "fs", mle_eval=R.exact_mle_eval)


def _equality_counts(fs, challenges):
    """over the tables of every bound round of the reference (challenges fixed): how often bind1 (field.hpp) meets the equality
    case of its three compares -- sub_mod(a1, a0) with a1 == a0, monty_reduce(r_m * diff) with the high word equal to the
    subtracted word (split into t == 0 and t != 0), add_mod(a0, prod) with a0 + prod == p -- restated in u64 numpy"""
    mask, MU = np.uint64(0xFFFFFFFF), np.uint64(0x88000001)
    sub = red0 = red = add = 0
    fs = [np.array(f, dtype=np.uint64) for f in fs]
    for ch in challenges:
        r_m = np.uint64((int(ch) << 32) % P)  # to_mont
        nxt = []
        for f in fs:
            h = len(f) // 2
            a0, a1 = f[:h], f[h:]
            sub += int(np.sum(a0 == a1))
            diff = (a1 + np.uint64(P) - a0) % np.uint64(P)
            t = r_m * diff  # < 2^31 * 2^31
            m = ((t & mask) * MU) & mask
            u = (m * np.uint64(P)) >> np.uint64(32)
            hi = t >> np.uint64(32)
            eq = hi == u
            red0 += int(np.sum(eq & (t == 0)))
            red += int(np.sum(eq & (t != 0)))
            prod = np.where(hi < u, hi + np.uint64(P) - u, hi - u)
            assert np.array_equal(prod, (np.uint64(int(ch)) * diff) % np.uint64(P))  # the restatement is mont_mul
            s = a0 + prod
            add += int(np.sum(s == np.uint64(P)))
            nxt.append(np.where(s >= np.uint64(P), s - np.uint64(P), s))
        fs = nxt
    return sub, red0, red, add


def test_edge_inputs_reach_the_equality_cases():
    """the compares of add_mod, sub_mod and monty_reduce at equality, counted at 2^11 over the bind of every round:
      sub_mod   a == b at every pair of a constant table (all_pm1, any challenge: 2047 per factor)
      add_mod   a + b == p at all 1024 pairs of step_down's first bind with challenge 1: (p - 1) + 1 * (0 - (p - 1)) = p
      monty_reduce  hi == u only with t == 0 (both words 0): r_m, diff < p and p is prime, so r_m * diff is no other multiple of
                p; reached wherever diff == 0 (constant tables) or the challenge is 0"""
    nv = 11
    one, zero, rnd = (R.edge_challenges(c, nv) for c in ("one", "zero", "random"))
    sub, red0, red, add = _equality_counts([R.pattern("all_pm1", nv)], rnd)
    assert (sub, red0, red, add) == (2047, 2047, 0, 0)
    sub, red0, red, add = _equality_counts([R.pattern("step_down", nv)], one)
    assert add == 1024 and sub == 1023 and red == 0  # the first bind; afterwards the table is all 0
    sub, red0, red, add = _equality_counts([R.pattern("random", nv)], zero)
    assert red0 == 2047 and add == 0
    # and no listed input reaches hi == u with t != 0
    tabs = _edge_tables(nv)
    total = [0, 0, 0, 0]
    for names, cname in R.edge_cases(nv):
        ch = R.edge_challenges(cname, nv)
        if ch is None:
            ch = R.prove([tabs[n] for n in names])[2]
        total = [x + y for x, y in zip(total, _equality_counts([tabs[n] for n in names], ch))]
    print("equality cases over the 126 edge inputs at 2^11: sub_mod a == b %d, monty_reduce t == 0 %d, t != 0 %d, add_mod == p %d"
          % tuple(total))
    assert total[0] > 0 and total[1] > 0 and total[2] == 0 and total[3] > 0
    # ... so one constructed input does (R.REDUCE_EDGE, d = 2): round 0's c_0 terms a0 a1 of a lane of k_product_sums at 2^11 -- the
    # four index pairs 4t .. 4t + 3 of one 16-byte vector -- added as low and high words (pd_add); the lane's monty_reduce(lo)
    a0, a1 = (tabs[n][:1 << (nv - 1)] for n in R.REDUCE_EDGE)
    pr = a0 * a1
    lo = (pr & np.uint64(0xFFFFFFFF)).reshape(-1, 4).sum(axis=1)
    hi = (pr >> np.uint64(32)).reshape(-1, 4).sum(axis=1)
    u = ((((lo & np.uint64(0xFFFFFFFF)) * np.uint64(0x88000001)) & np.uint64(0xFFFFFFFF)) * np.uint64(P)) >> np.uint64(32)
    assert len(lo) == 256 and np.all(lo == 2 * P) and np.all(hi == 0) and np.all(lo >> np.uint64(32) == u) and np.all(u == 0)


def test_entries_in_header_binding_ctypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "zig", "zigz_hip.zig")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert f'pub extern "c" fn {name}(' in zig, name
    assert re.search(r"#define ZIGZ_PRODUCT_MAX_DEGREE 3\b", hdr) and re.search(r"#define ZIGZ_PRODUCT_MAX_LOG2_N 30\b", hdr)
    assert re.search(r"#define ZIGZ_ABI_VERSION 1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name in ENTRIES:
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == 12
    assert _ffi.lib.zigz_abi_version() == 1
    for m in ("dev_sumcheck_prove_product_batch", "sumcheck_prove_product_batch"):
        assert callable(getattr(hip.Context, m))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pd") / "product_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_driver", "product_host.cpp")] + srcs + ["-o", exe])
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


def test_driver_proofs_equal_the_reference(driver, tmp_path):
    """tables of 2 .. 1024 values, d = 1..3, Fiat-Shamir and fixed challenges; extreme tables (all p - 1; low half 0, high half
    p - 1: every term maximal); one table as all factors.  Both of the driver's provers -- the host's tail rounds, and the rounds
    assembled from kernel-style sums -- print the reference's proof."""
    cases = []
    for v in range(1, 11):
        for d in (1, 2, 3):
            fs = tables(7400 + 10 * v + d, d, 1 << v)
            cases.append((fs, None))
            if v in (1, 4, 10):
                cases.append((fs, O.splitmix64_field(7500 + v, v)))
    for d in (2, 3):
        top = np.full(1 << 10, P - 1, dtype=np.uint64)
        cases.append(([top] * d, None))
        step = np.concatenate([np.zeros(1 << 9, dtype=np.uint64), np.full(1 << 9, P - 1, dtype=np.uint64)])
        cases.append(([step] * d, None))
        f = O.splitmix64_field(7600 + d, 1 << 6)
        cases.append(([f] * d, None))
    path = tmp_path / "instances.txt"
    with open(path, "w") as fh:
        for fs, ch in cases:
            words = [len(fs), len(fs[0]), 0 if ch is None else 1] + [int(x) for f in fs for x in f] + ([] if ch is None else [int(x) for x in ch])
            fh.write(" ".join(str(w) for w in words) + "\n")
    lines = _run(driver, "prove", str(path)).split("\n")[:-1]
    assert len(lines) == 2 * len(cases)
    for i, (fs, ch) in enumerate(cases):
        d, v = len(fs), len(fs[0]).bit_length() - 1
        ref = R.prove(fs, ch)
        for which, line in zip(("tail", "sums"), lines[2 * i: 2 * i + 2]):
            w = [int(x) for x in line.split()]
            assert len(w) == 2 + (d + 1) * v + v + d
            got = (w[0], w[2: 2 + (d + 1) * v], w[2 + (d + 1) * v: 2 + (d + 2) * v], w[2 + (d + 2) * v:], w[1])
            assert R.same(got, ref), (which, d, v, ch is not None)


def _driver_case_lines(cases):
    return [" ".join(str(w) for w in [len(fs), len(fs[0]), 0 if ch is None else 1] + [int(x) for f in fs for x in f]
                     + ([] if ch is None else [int(x) for x in ch])) for fs, ch in cases]


def test_driver_edge_inputs(driver, tmp_path):
    """the edge pattern sets at 2^10 with the challenges 0, 1 and p - 1: coefficients() over kernel-style sums and tail_rounds()
    see the inputs of test_gpu_sumcheck_product_exact.py's field-edge cases, under the sanitizers"""
    nv = 10
    tabs = _edge_tables(nv)
    cases = [([tabs[n] for n in ps[:d]], R.edge_challenges(c, nv)) for ps in R.PATTERN_SETS for d in (1, 2, 3)
             for c in ("zero", "one", "pm1")] + [([tabs[n] for n in R.REDUCE_EDGE], None)]
    path = tmp_path / "edges.txt"
    path.write_text("\n".join(_driver_case_lines(cases)) + "\n")
    lines = _run(driver, "prove", str(path)).split("\n")[:-1]
    assert len(lines) == 2 * len(cases) == 128
    for i, (fs, ch) in enumerate(cases):
        d = len(fs)
        ref = R.prove(fs, ch)
        for which, line in zip(("tail", "sums"), lines[2 * i: 2 * i + 2]):
            w = [int(x) for x in line.split()]
            assert len(w) == 2 + (d + 1) * nv + nv + d
            got = (w[0], w[2: 2 + (d + 1) * nv], w[2 + (d + 1) * nv: 2 + (d + 2) * nv], w[2 + (d + 2) * nv:], w[1])
            assert R.same(got, ref), (which, i)


def test_argument_checker(driver):
    got = {}
    for line in _run(driver, "check").split("\n")[:-1]:
        name, st, bad, written = line.split()
        got[name] = (int(st), int(bad), int(written))
    expect = {}
    for s in ("host", "dev"):
        w = 1 if s == "host" else 0  # the driver proves only the host form's batches (there is no device)
        expect.update({
            f"ok_{s}": (OK, -1, w), f"ok_fixed_{s}": (OK, -1, w), f"k0_{s}": (OK, -1, 0), f"k4097_{s}": (INVALID, -1, 0),
            f"degree0_1_{s}": (INVALID, 1, 0), f"degree4_2_{s}": (INVALID, 2, 0),
            f"null_factor_1_{s}": (INVALID, 1, 0), f"null_factor_2_{s}": (INVALID, 2, 0),
            f"n0_0_{s}": (EMPTY, 0, 0), f"n1_1_{s}": (NO_VARIABLES, 1, 0), f"n3_1_{s}": (NOT_POW2, 1, 0),
            f"n12_2_{s}": (NOT_POW2, 2, 0), f"n2p31_2_{s}": (INVALID, 2, 0),
            f"challenge_1_{s}": (NOT_CANONICAL, 1, 0), f"challenge_p_minus_1_{s}": (OK, -1, w),
            f"no_degrees_{s}": (INVALID, -1, 0), f"no_ns_{s}": (INVALID, -1, 0), f"no_claimed_{s}": (INVALID, -1, 0),
            f"no_rounds_{s}": (INVALID, -1, 0), f"no_points_{s}": (INVALID, -1, 0), f"no_factor_evals_{s}": (INVALID, -1, 0),
            f"no_finals_{s}": (INVALID, -1, 0),
        })
    expect.update({
        "misaligned_1_dev": (INVALID, 1, 0), "value_1_host": (NOT_CANONICAL, 1, 0),
        # the calls in order would have stopped at the table with the value >= p: it is reported, not the later shape
        "value_0_before_n12_2_host": (NOT_CANONICAL, 0, 0), "n3_1_before_value_2_host": (NOT_POW2, 1, 0),
        "value_past_the_table_host": (OK, -1, 1),
    })
    assert got == expect, {k: (got.get(k), expect.get(k)) for k in set(got) | set(expect) if got.get(k) != expect.get(k)}


def test_product_kernels_use_no_scratch_and_count_behind_a_barrier():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import isa_counts
    from test_isa_handoff import handoffs
    asm = isa_counts.assembly(sources=("sumcheck_product.hip",))
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    assert len(names) == 4 and len(sizes) == 4, names  # k_product_sums, k_product_bind, k_product_finish, k_product_tails
    assert all(int(s) == 0 for s in sizes), dict(zip(names, sizes))
    found = handoffs(asm)
    assert {k for k, _, _ in found} == {"k_product_finish", "k_product_tails"}, found
    assert all(barrier for _, _, barrier in found), found
    # the tables are read with 16-byte non-temporal loads
    assert len(re.findall(r"_load_dwordx4 .* nt\b", asm)) >= 12
