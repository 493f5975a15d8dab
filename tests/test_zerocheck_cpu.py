"""The batched eq tables and the batched product-proof verification without a GPU: the four entries in the header, the ctypes
table, the Zig binding and the library; the numpy restatement (zerocheck_ref.py) pinned against the oracle; the host header
(product_verify_host.hpp: argument checks and their order, the replay with d + 1 coefficients, eq_at, the verdict) built with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone driver (tests/c_driver/product_verify_host.cpp) and run as a
child process against the reference; the tamper set of the GPU tests rejected by the reference alone; the gfx950 assembly of
eq_batch.hip (no scratch, 16-byte stores)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import sumcheck_product_ref as R
import sumcheck_verify_ref as L
import zerocheck_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
ENTRIES = {"zigz_dev_eq_table_batch": 6, "zigz_eq_table_batch": 6, "zigz_dev_sumcheck_verify_product_batch": 18,
           "zigz_sumcheck_verify_product_batch": 18}
OK, EMPTY, NOT_POW2, NO_VARIABLES, NOT_CANONICAL, INVALID = 0, 1, 2, 5, 102, 103
VS = [1, 2, 5, 11]


def test_entries_in_header_binding_ctypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "zig", "zigz_hip.zig")).read()
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert f'pub extern "c" fn {name}(' in zig, name
    assert re.search(r"#define ZIGZ_FACTOR_TABLE 0\b", hdr) and re.search(r"#define ZIGZ_FACTOR_EQ 1\b", hdr)
    assert re.search(r"#define ZIGZ_ABI_VERSION 1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name, nargs in ENTRIES.items():
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == nargs
    assert _ffi.lib.zigz_abi_version() == 1
    for m in ("eq_table_batch", "dev_eq_table_batch", "sumcheck_verify_product_batch", "dev_sumcheck_verify_product_batch"):
        assert callable(getattr(hip.Context, m))


def _taus(v):
    """random, all 0, all 1, all p - 1, a 0/1 pattern, a mix of the edge values"""
    rnd = [int(x) for x in O.splitmix64_field(8000 + v, v)]
    bits = [(j * 5 + 1) % 3 % 2 for j in range(v)]
    return {"random": rnd, "zero": [0] * v, "one": [1] * v, "pm1": [P - 1] * v, "bits": bits, "mix": [(0, 1, P - 1)[j % 3] for j in range(v)]}


@pytest.mark.parametrize("v", VS)
def test_eq_table_against_the_oracle(v):
    n = 1 << v
    t = O.splitmix64_field(8100 + v, n)
    q = [int(x) for x in O.splitmix64_field(8200 + v, v)]
    for name, tau in _taus(v).items():
        e = Z.eq_table(tau)
        assert len(e) == n and int(e.max()) < P
        assert int(np.sum(e, dtype=np.uint64)) % P == 1, name
        assert Z.dot(e, t) == O.mle_eval(P, t, tau), name
        assert Z.eq_at(tau, q) == O.mle_eval(P, e, q), name
        if name in ("zero", "one", "bits"):  # tau in {0,1}^v: the indicator of the index whose bit j is tau_j
            ind = np.zeros(n, dtype=np.uint64)
            ind[sum(b << j for j, b in enumerate(tau))] = 1
            assert np.array_equal(e, ind), name
    assert list(Z.eq_table([])) == [1]


@pytest.mark.parametrize("v", VS)
def test_eq_factor_in_the_reference_prover(v):
    n = 1 << v
    tau = [int(x) for x in O.splitmix64_field(8300 + v, v)]
    e = Z.eq_table(tau)
    f, g = O.splitmix64_field(8400 + v, n), O.splitmix64_field(8500 + v, n)
    claimed, rounds, point, evals, fe = R.prove([e, f, g])
    rev = [int(x) for x in point][::-1]
    assert int(evals[0]) == Z.eq_at(tau, rev)
    assert Z.verdict([Z.Eq(tau), f, g], (claimed, rounds, point, evals, fe), reversed_point=True)[0]
    # a zero-check: a 0/1 table satisfies g (g - 1) = 0 on the whole cube
    bits = O.splitmix64_field(8600 + v, n) & np.uint64(1)
    proof = R.prove([e, bits, (bits + np.uint64(P - 1)) % np.uint64(P)])
    assert proof[0] == 0
    assert Z.verdict([Z.Eq(tau), bits, (bits + np.uint64(P - 1)) % np.uint64(P)], proof, reversed_point=True)[0]


def test_reference_verdict_at_degree_one_is_the_linear_one():
    for v in VS:
        t = O.splitmix64_field(8700 + v, 1 << v)
        claimed, rounds, point, evals, fe = R.prove([t])
        for kind, c, r, q, f in L.tampered(claimed, rounds, point, fe):
            for rev in (False, True):
                want = L.verdict(t, c, r, q, f, reversed_point=rev)
                got = Z.verdict([t], (c, r, q, evals, f), reversed_point=rev, check_factor_evals=False)
                assert (got[0], got[1], got[2][0]) == want, (v, kind, rev)


@pytest.mark.parametrize("v", [11, 14])
def test_every_tamper_is_rejected_by_the_reference(v):
    """the instances of the GPU tamper tests: none is left out, so those tests cannot pass vacuously"""
    factors, proof, other, other_tau = Z.pinned_zero_check(v)
    assert proof[0] == 0 and Z.verdict(factors, proof, reversed_point=True)[0]
    cases = Z.tampered(factors, proof, other, other_tau)
    assert tuple(cases) == Z.TAMPERS and len(cases) == 10
    for name, (fs, pr) in cases.items():
        assert not Z.verdict(fs, pr, reversed_point=True)[0], name
    # factor_eval is caught by the factor evals alone: without them the proof is the honest one
    fs, pr = cases["factor_eval"]
    assert Z.verdict(fs, pr, reversed_point=True, check_factor_evals=False)[0]


# ---------------------------------------------------------------- the host header under the sanitizers
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pv") / "product_verify_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_driver", "product_verify_host.cpp")] + srcs + ["-o", exe])
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


def test_driver_verdicts_equal_the_reference(driver, tmp_path):
    """d = 1, 2, 3 at v = 1, 2, 5, 11, with and without an eq first factor, under both point orders, honest and with every word
    tamper: the driver's replay, eq_at and verdict print the reference's verdict, expected eval and oracle evals; at d = 1
    pv::replay_rounds equals sv::replay_rounds word for word"""
    cases = []  # (factors, proof, reversed, check_factor_evals)
    for v in VS:
        n = 1 << v
        for d in (1, 2, 3):
            tabs = [O.splitmix64_field(8800 + 10 * v + d + 3 * j, n) for j in range(d)]
            for with_eq in (False, True):
                tau = [int(x) for x in O.splitmix64_field(8900 + v + d, v)]
                fs = ([Z.Eq(tau)] + tabs[1:]) if with_eq else tabs
                proof = R.prove(Z.materialise(fs))
                claimed, rounds, point, evals, fe = proof
                variants = [proof]
                for w in (0, (d + 1) * (v // 2) + d, (d + 1) * v - 1):
                    bad = rounds.copy()
                    bad[w] = (int(bad[w]) + 1) % P
                    variants.append((claimed, bad, point, evals, fe))
                variants.append(((claimed + 1) % P, rounds, point, evals, fe))
                variants.append((claimed, rounds, point, evals, (fe + 1) % P))
                bad = evals.copy()
                bad[0] = (int(bad[0]) + 1) % P
                variants.append((claimed, rounds, point, bad, fe))
                for pr in variants:
                    for rev in (False, True):
                        cases.append((fs, pr, rev, True))
                cases.append((fs, variants[-1], True, False))
    lines = []
    want = []
    for fs, (claimed, rounds, point, evals, fe), rev, cfe in cases:
        d, v = len(fs), len(point)
        ok, expected, orc = Z.verdict(fs, (claimed, rounds, point, evals, fe), reversed_point=rev, check_factor_evals=cfe)
        want.append((int(ok), expected, orc))
        words = [d, v, int(rev), int(cfe), int(claimed), int(fe)] + [int(x) for x in rounds] + [int(x) for x in point] + [int(x) for x in evals]
        for f, o in zip(fs, orc):
            words += [1] + f.tau if isinstance(f, Z.Eq) else [0, o]
        lines.append(" ".join(str(w) for w in words))
    path = tmp_path / "proofs.txt"
    path.write_text("\n".join(lines) + "\n")
    out = _run(driver, "verify", str(path)).split("\n")[:-1]
    assert len(out) == len(cases)
    accepted = 0
    for (fs, pr, rev, cfe), w, line in zip(cases, want, out):
        got = [int(x) for x in line.split()]
        d = len(fs)
        assert (got[0], got[2], got[3: 3 + d]) == w, (d, len(pr[2]), rev, cfe)
        assert got[1] == R.claim_chain(pr[0], pr[1], len(pr[2]), d)[0]
        if d == 1:
            assert got[4] == 1
        accepted += got[0]
    assert 0 < accepted < len(cases)


def test_argument_checker(driver):
    got = {}
    for line in _run(driver, "check").split("\n")[:-1]:
        name, st, bad = line.split()
        got[name] = (int(st), int(bad))
    expect = {}
    for s in ("host", "dev"):
        expect.update({
            f"eq_ok_{s}": (OK, -1), f"eq_k0_{s}": (OK, -1), f"eq_k4097_{s}": (INVALID, -1), f"eq_no_points_{s}": (INVALID, -1),
            f"eq_n0_{s}": (EMPTY, 1), f"eq_n1_{s}": (OK, -1), f"eq_n3_{s}": (NOT_POW2, 1), f"eq_n{1 << 33}_{s}": (INVALID, 1),
            f"eq_point3_{s}": (NOT_CANONICAL, 3), f"eq_ignores_rounds_{s}": (OK, -1),
            f"verify_ok_{s}": (OK, -1), f"verify_reversed_ok_{s}": (OK, -1), f"verify_flag2_{s}": (INVALID, -1),
            f"verify_k0_{s}": (OK, -1), f"verify_k4097_{s}": (INVALID, -1), f"verify_no_rejected_{s}": (INVALID, -1),
            f"verify_no_fevals_ok_{s}": (OK, -1), f"verify_no_kinds_null1_{s}": (INVALID, 1), f"verify_no_taus1_{s}": (INVALID, 1),
            f"verify_n0_{s}": (EMPTY, 1), f"verify_n1_{s}": (NO_VARIABLES, 1), f"verify_n3_{s}": (NOT_POW2, 1),
            f"verify_degree0_2_{s}": (INVALID, 2), f"verify_degree4_2_{s}": (INVALID, 2), f"verify_kind2_2_{s}": (INVALID, 2),
            f"verify_eq_with_pointer3_{s}": (INVALID, 3), f"verify_point3_{s}": (NOT_CANONICAL, 3),
            f"verify_round1_{s}": (NOT_CANONICAL, 1), f"verify_claimed2_{s}": (NOT_CANONICAL, 2), f"verify_final0_{s}": (NOT_CANONICAL, 0),
            f"verify_feval2_{s}": (NOT_CANONICAL, 2), f"verify_feval2_unread_{s}": (OK, -1), f"verify_tau3_{s}": (NOT_CANONICAL, 3),
            # the first failing proof wins, whatever its kind of failure
            f"verify_first_of_two_{s}": (NOT_CANONICAL, 1), f"verify_round2_before_n12_3_{s}": (NOT_CANONICAL, 2),
            f"verify_n3_2_before_tau3_{s}": (NOT_POW2, 2), f"verify_p_minus_1_{s}": (OK, -1),
        })
    expect.update({
        # the calls in order would have stopped at the table with the value >= p: it is reported, not the later shape
        "verify_value1_before_n12_3_host": (NOT_CANONICAL, 1), "verify_n3_2_before_value3_host": (NOT_POW2, 2),
        "verify_eq_slot_unread_host": (NOT_POW2, 3),
        "eq_null3_host": (INVALID, 3), "eq_misaligned1_dev": (INVALID, 1), "eq_null0_dev": (INVALID, 0),
        "verify_misaligned2_dev": (INVALID, 2), "verify_null0_dev": (INVALID, 0), "verify_null0_host": (INVALID, 0),
    })
    assert got == expect, {k: (got.get(k), expect.get(k)) for k in set(got) | set(expect) if got.get(k) != expect.get(k)}


def test_eq_kernel_uses_no_scratch_and_stores_16_bytes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    asm = isa_counts.assembly(sources=("eq_batch.hip",))
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    assert len(names) == 1 and "k_eq_batch_expand" in names[0] and sizes == ["0"], (names, sizes)
    counts = isa_counts.count(asm)["k_eq_batch_expand"]
    lds = re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)
    print("k_eq_batch_expand: %d VGPRs, %s bytes of LDS" % (counts["vgprs"], lds[0]))
    assert len(re.findall(r"global_store_dwordx4 ", asm)) == 8  # one 16-byte store per lane and loop step
    assert not re.search(r"_atomic_", asm)  # nothing is counted or published: the launch is left queued
