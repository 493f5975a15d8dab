"""The zero-check sumcheck with the eq factor in closed form, without a GPU: the four entries in the header, the Zig binding, the
ctypes table and the library; the reference adapter (zerocheck_closed_ref.py) against the product reference; the host header
(zerocheck_host.hpp: argument checks, prefix scalar, linear factor, weights, tail rounds, verdict) built with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone driver (tests/c_driver/zerocheck_host.cpp) and run as a child process against the
reference; the gfx950 assembly of sumcheck_zerocheck.hip (no scratch, LDS within bounds, 16-byte accesses)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import sop_ref as S
import sumcheck_product_ref as R
import zerocheck_closed_ref as ZC
import zerocheck_ref as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
ENTRIES = {"zigz_dev_sumcheck_prove_zerocheck_batch": 18, "zigz_sumcheck_prove_zerocheck_batch": 18,
           "zigz_dev_sumcheck_verify_zerocheck_batch": 22, "zigz_sumcheck_verify_zerocheck_batch": 22}
OK, EMPTY, NOT_POW2, NO_VARIABLES, NOT_CANONICAL, INVALID = 0, 1, 2, 5, 102, 103
SPECIAL_TAU = [0, 1, (P + 1) // 2, P - 1]


def pool(seed, M, n):
    return [O.splitmix64_field(seed + 17 * j, n) for j in range(M)]


def mixed_tau(seed, v):
    """random words with 0, 1, (p + 1) / 2 and p - 1 mixed in, a different place for every seed"""
    tau = [int(x) for x in O.splitmix64_field(seed, v)]
    for j in range(v):
        if (j + seed) % 3 == 0:
            tau[j] = SPECIAL_TAU[(j + seed) // 3 % 4]
    return tau


def test_entries_in_header_binding_ctypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "zig", "zigz_hip.zig")).read()
    for name, arity in ENTRIES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert m and m.group(1).count(",") + 1 == arity, name
        z = re.search(r'pub extern "c" fn %s\(([^;]*)\) ' % name, zig)
        assert z and z.group(1).count(":") == arity, name
    assert re.search(r"#define ZIGZ_ZEROCHECK_MAX_DEGREE 4\b", hdr) and re.search(r"#define ZIGZ_PRODUCT_MAX_DEGREE 3\b", hdr)
    assert re.search(r"#define ZIGZ_ABI_VERSION 1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name, arity in ENTRIES.items():
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == arity
    assert _ffi.lib.zigz_abi_version() == 1
    for m in ("dev_sumcheck_prove_zerocheck_batch", "sumcheck_prove_zerocheck_batch", "dev_sumcheck_verify_zerocheck_batch",
              "sumcheck_verify_zerocheck_batch"):
        assert callable(getattr(hip.Context, m))


@pytest.mark.parametrize("v", [1, 4, 9])
def test_reference_adapter_is_the_product_reference_with_eq_as_a_factor(v):
    """one term, alpha = 1: the product reference's proof of [f_0, .., eq]; the claimed sum is the eq-weighted sum of C"""
    tau = mixed_tau(v, v)
    for d in (1, 2, 3):
        fs = pool(9700 + 10 * v + d, d, 1 << v)
        got = ZC.prove(fs, [(1, tuple(range(d)))], tau)
        want = R.prove(fs + [Z.eq_table(tau)])
        assert ZC.same(got, ZC.from_sop(want, d))
        assert len(got[1]) == (d + 2) * v
        prod = np.ones(1 << v, dtype=np.uint64)
        for f in fs:
            prod = prod * f % np.uint64(P)
        assert got[0] == Z.dot(Z.eq_table(tau), prod)
        assert got[4] == Z.eq_at(tau, [int(x) for x in got[2]][::-1])
        assert ZC.verdict(fs, [(1, tuple(range(d)))], tau, got)[0]


def test_replay_at_five_coefficients_and_a_pinned_seed_exists():
    """the claim chain is generic in the degree: a degree-4 round polynomial (deg C = 3) replays, a changed word does not; and among
    the first few seeds there is one at which the reference rejects every tamper at 2^12 (the GPU file uses it)"""
    v = 6
    fs, tau = pool(9800, 3, 1 << v), mixed_tau(5, v)
    terms = [(7, (0, 1, 2)), (P - 1, (2, 2)), (3, (1,))]
    proof = ZC.prove(fs, terms, tau)
    assert len(proof[1]) == 5 * v
    ok, expected, drawn = R.claim_chain(proof[0], proof[1], v, 4)
    assert ok and expected == proof[5] and drawn == [int(x) for x in proof[2]]
    bad = proof[1].copy()
    bad[5 * 3 + 4] = (int(bad[5 * 3 + 4]) + 1) % P
    ok, expected, _ = R.claim_chain(proof[0], bad, v, 4)
    assert not (ok and expected == proof[5])
    pl, tm, tau, proof, other = ZC.pinned(12)
    assert ZC.verdict(pl, tm, tau, proof)[0]
    assert set(ZC.tampered(pl, tm, tau, proof, other)) == set(ZC.TAMPERS)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zerocheck") / "zerocheck_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_driver", "zerocheck_host.cpp")] + srcs + ["-o", exe])
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


def _line(fs, terms, tau, ch):
    words = [len(fs), len(fs[0]), len(terms), 0 if ch is None else 1]
    for alpha, idx in terms:
        words += [int(alpha), len(idx)] + [int(i) for i in idx]
    words += [int(t) for t in tau]
    words += [int(x) for f in fs for x in f] + ([] if ch is None else [int(x) for x in ch])
    return " ".join(str(w) for w in words)


@pytest.fixture(scope="module")
def cases():
    """v = 1..10 crossed with (M, T) in {1, 4, 8} x {1, 3, 8} (sop_ref.structure: mixed degrees up to 3, i.e. rounds of up to 5
    coefficients); taus mixed from random words and 0, 1, (p + 1) / 2, p - 1; some with fixed challenges; saturated tables"""
    out = []
    for v in range(1, 11):
        for M in (1, 4, 8):
            for T in (1, 3, 8):
                fs = pool(9400 + 100 * v + 10 * M + T, M, 1 << v)
                terms = S.structure(M, T, seed=v + M + T)
                tau = mixed_tau(v + M + T, v)
                out.append((fs, terms, tau, None))
                if v in (1, 4, 10) and T == 3:
                    out.append((fs, terms, tau, O.splitmix64_field(9500 + v, v)))
    top = [np.full(1 << 10, P - 1, dtype=np.uint64)] * 3
    cubic = [(P - 1, (t % 3, (t + 1) % 3, (t + 2) % 3)) for t in range(8)]
    for tau in ([P - 1] * 10, [0] * 10, [1] * 10, [(P + 1) // 2] * 10):
        out.append((top, cubic, tau, None))
    assert any(S.degree(t) == 3 for _, t, _, _ in out)
    assert {x for _, _, tau, _ in out for x in tau} >= set(SPECIAL_TAU)
    return out, [ZC.prove(*c) for c in out]


@pytest.mark.parametrize("L", [2, 5])
def test_driver_proofs_equal_the_reference(driver, cases, tmp_path, L):
    """Both of the driver's provers -- the host's weighted tail rounds from the full tables, and the rounds of 2^L pairs or more
    assembled from kernel-style weighted class sums (lo, the hi stages and the per-block partials formed as the kernels form
    them) through the host's coefficient assembly -- print the reference's proof, and the verdict accepts it and rejects a
    changed final eval or eq eval."""
    cs, refs = cases
    path = tmp_path / "instances.txt"
    path.write_text("\n".join(_line(*c) for c in cs) + "\n")
    lines = _run(driver, "prove", str(path), str(L)).split("\n")[:-1]
    assert len(lines) == 3 * len(cs)
    for i, ((fs, terms, tau, ch), ref) in enumerate(zip(cs, refs)):
        d, v, M = S.degree(terms), len(tau), len(fs)
        for which, line in zip(("tail", "sums"), lines[3 * i: 3 * i + 2]):
            w = [int(x) for x in line.split()]
            assert len(w) == 3 + (d + 2) * v + v + M
            got = (w[0], w[3: 3 + (d + 2) * v], w[3 + (d + 2) * v: 3 + (d + 3) * v], w[3 + (d + 3) * v:], w[2], w[1])
            assert ZC.same(got, ref), (which, i, M, len(terms), v, ch is not None)
        if ch is None:
            assert lines[3 * i + 2] == "1 0 0", (i, lines[3 * i + 2])


def test_argument_checkers(driver):
    got = {}
    for line in _run(driver, "check").split("\n")[:-1]:
        name, st, bad = line.split()
        got[name] = (int(st), int(bad))
    expect = {}
    for s in ("host", "dev"):
        expect.update({
            f"ok_{s}": (OK, -1), f"ok_fixed_{s}": (OK, -1), f"k0_{s}": (OK, -1), f"k0_no_eq_points_{s}": (OK, -1),
            f"k4097_{s}": (INVALID, -1),
            f"pool0_1_{s}": (INVALID, 1), f"pool9_2_{s}": (INVALID, 2), f"terms0_0_{s}": (INVALID, 0), f"terms9_1_{s}": (INVALID, 1),
            f"degree0_0_{s}": (INVALID, 0), f"degree4_2_{s}": (INVALID, 2), f"index2_0_{s}": (INVALID, 0), f"index3_1_{s}": (INVALID, 1),
            f"null_table_1_{s}": (INVALID, 1), f"n0_0_{s}": (EMPTY, 0), f"n1_1_{s}": (NO_VARIABLES, 1), f"n3_1_{s}": (NOT_POW2, 1),
            f"n12_2_{s}": (NOT_POW2, 2), f"n2p31_2_{s}": (INVALID, 2), f"challenge_1_{s}": (NOT_CANONICAL, 1),
            f"coeff_1_{s}": (NOT_CANONICAL, 1),
            f"tau_0_{s}": (NOT_CANONICAL, 0), f"tau_1_{s}": (NOT_CANONICAL, 1), f"tau_2_{s}": (NOT_CANONICAL, 2),
            f"n3_1_before_tau_1_{s}": (NOT_POW2, 1), f"tau_0_before_n3_1_{s}": (NOT_CANONICAL, 0),
            f"n3_1_before_tau_2_{s}": (NOT_POW2, 1), f"tau_0_before_coeff_1_{s}": (NOT_CANONICAL, 0),
            f"no_n_tables_{s}": (INVALID, -1), f"no_ns_{s}": (INVALID, -1), f"no_coeffs_{s}": (INVALID, -1),
            f"no_eq_points_{s}": (INVALID, -1), f"no_eq_evals_{s}": (INVALID, -1), f"no_table_evals_{s}": (INVALID, -1),
            f"no_finals_{s}": (INVALID, -1),
            f"verify_ok_{s}": (OK, -1), f"verify_ok_flags0_{s}": (OK, -1), f"verify_flags2_{s}": (INVALID, -1),
            f"verify_no_n_rejected_{s}": (INVALID, -1), f"verify_k0_{s}": (OK, -1), f"verify_no_eq_points_{s}": (INVALID, -1),
            f"verify_no_evals_is_ok_{s}": (OK, -1), f"verify_no_finals_{s}": (INVALID, -1), f"verify_degree4_2_{s}": (INVALID, 2),
            f"verify_n1_1_{s}": (NO_VARIABLES, 1), f"verify_tau_1_{s}": (NOT_CANONICAL, 1), f"verify_eq_eval_2_{s}": (NOT_CANONICAL, 2),
            f"verify_round_word_0_last_{s}": (NOT_CANONICAL, 0), f"verify_round_word_1_last_{s}": (NOT_CANONICAL, 1),
            f"verify_round_word_2_last_{s}": (NOT_CANONICAL, 2), f"verify_word_behind_the_rounds_{s}": (OK, -1),
            f"verify_point_1_{s}": (NOT_CANONICAL, 1),
        })
    expect.update({
        "misaligned_1_dev": (INVALID, 1), "value_1_host": (NOT_CANONICAL, 1),
        "value_0_before_tau_1_host": (NOT_CANONICAL, 0), "tau_1_before_value_2_host": (NOT_CANONICAL, 1),
    })
    assert got == expect, {k: (got.get(k), expect.get(k)) for k in set(got) | set(expect) if got.get(k) != expect.get(k)}


def test_zerocheck_pass_kernels_use_no_scratch_and_move_16_bytes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    asm = isa_counts.assembly(sources=("sumcheck_zerocheck.hip",))
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)]
    assert len(names) == 2 and len(scratch) == 2 and len(lds) == 2, names  # k_zc_sums, k_zc_bind
    counts = isa_counts.count(asm)
    for k in ("k_zc_sums", "k_zc_bind"):
        i = next(j for j, n in enumerate(names) if k in n)
        print("%s: %d VGPRs, %d bytes of LDS, %d bytes of scratch" % (k, counts[k]["vgprs"], lds[i], scratch[i]))
        assert scratch[i] == 0
        assert lds[i] <= 32 * 1024
    # the pass loads and stores are 16 bytes wide: no narrower access to global memory but the partial sums', the descriptor's and
    # the trip's one hi word
    body = {k: asm[asm.index("\n_ZN2zk9%sE" % k): asm.index(".Lfunc_end", asm.index("\n_ZN2zk9%sE" % k))] for k in ("k_zc_sums", "k_zc_bind")}
    for k, text in body.items():
        assert len(re.findall(r"global_load_dwordx4 ", text)) >= 8 * (2 if k == "k_zc_sums" else 4)
        assert not re.search(r"(global|flat)_load_(dword|dwordx2|dwordx3|ubyte|ushort) .*\bnt\b", text), k
    assert len(re.findall(r"global_store_dwordx4 ", body["k_zc_bind"])) >= 8 * 2
    assert not re.search(r"global_store_dwordx4 ", body["k_zc_sums"])
