"""The batched sum-of-products sumcheck without a GPU: the four entries in the header, the Zig binding, the ctypes table and the
library; the host header (sop_host.hpp: argument checks, class-to-coefficient assembly from kernel-style sums, tail rounds over a
pool with terms, the verifier's combination) built with AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone driver
(tests/c_driver/sop_host.cpp) and run as a child process against the reference (sop_ref.py); the reference against the product
reference at one term; the gfx950 assembly of sumcheck_sop.hip (no scratch, LDS within bounds, 16-byte accesses)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import sop_ref as S
import sumcheck_product_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
ENTRIES = {"zigz_dev_sumcheck_prove_sop_batch": 16, "zigz_sumcheck_prove_sop_batch": 16,
           "zigz_dev_sumcheck_verify_sop_batch": 22, "zigz_sumcheck_verify_sop_batch": 22}
OK, EMPTY, NOT_POW2, NO_VARIABLES, NOT_CANONICAL, INVALID = 0, 1, 2, 5, 102, 103


def pool(seed, M, n):
    return [O.splitmix64_field(seed + 17 * j, n) for j in range(M)]


def test_entries_in_header_binding_ctypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "zig", "zigz_hip.zig")).read()
    for name, arity in ENTRIES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert m and m.group(1).count(",") + 1 == arity, name
        z = re.search(r'pub extern "c" fn %s\(([^;]*)\) ' % name, zig)
        assert z and z.group(1).count(":") == arity, name
    assert re.search(r"#define ZIGZ_SOP_MAX_TABLES 8\b", hdr) and re.search(r"#define ZIGZ_SOP_MAX_TERMS 8\b", hdr)
    assert re.search(r"#define ZIGZ_ABI_VERSION 1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name, arity in ENTRIES.items():
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == arity
    assert _ffi.lib.zigz_abi_version() == 1
    for m in ("dev_sumcheck_prove_sop_batch", "sumcheck_prove_sop_batch", "dev_sumcheck_verify_sop_batch", "sumcheck_verify_sop_batch"):
        assert callable(getattr(hip.Context, m))


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("v", [1, 4, 11])
def test_reference_at_one_term_is_the_product_reference(d, v):
    """one term, alpha = 1, distinct tables: word for word sumcheck_product_ref.prove"""
    fs = pool(9000 + 10 * v + d, d, 1 << v)
    terms = [(1, tuple(range(d)))]
    assert S.same(S.prove(fs, terms), R.prove(fs))
    ch = O.splitmix64_field(9100 + v, v)
    assert S.same(S.prove(fs, terms, ch), R.prove(fs, ch))


@pytest.mark.parametrize("M,T", [(1, 1), (4, 3), (8, 8)])
def test_reference_proofs_verify(M, T):
    v = 9
    fs = pool(9200 + M, M, 1 << v)
    terms = S.structure(M, T, seed=M + T)
    proof = S.prove(fs, terms)
    assert proof[0] == S.claimed_sum(fs, terms)
    S.check_proof(fs, terms, proof)
    S.check_proof(fs, terms, S.prove(fs, terms, O.splitmix64_field(9300 + M, v)), fiat_shamir=False)
    bad = proof[1].copy()
    bad[len(bad) // 2] = (int(bad[len(bad) // 2]) + 1) % P
    ok, expected, _ = R.claim_chain(proof[0], bad, v, S.degree(terms))
    assert not (ok and expected == proof[4])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sop") / "sop_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_driver", "sop_host.cpp")] + srcs + ["-o", exe])
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout


def _line(fs, terms, ch):
    words = [len(fs), len(fs[0]), len(terms), 0 if ch is None else 1]
    for alpha, idx in terms:
        words += [int(alpha), len(idx)] + [int(i) for i in idx]
    words += [int(x) for f in fs for x in f] + ([] if ch is None else [int(x) for x in ch])
    return " ".join(str(w) for w in words)


def test_driver_proofs_equal_the_reference(driver, tmp_path):
    """v = 1..10 crossed with (M, T) in {1, 4, 8} x {1, 3, 8}: mixed degrees, a repeated index, an unused table and alphas 0, 1,
    p - 1 and random (sop_ref.structure); Fiat-Shamir and fixed challenges; all-(p - 1) tables with 8 cubic terms of alpha p - 1.
    Both of the driver's provers -- the host's tail rounds and the rounds assembled from kernel-style class sums -- print the
    reference's proof, and the verifier's combination accepts it and rejects a changed final eval or table eval."""
    cases = []
    for v in range(1, 11):
        for M in (1, 4, 8):
            for T in (1, 3, 8):
                fs = pool(9400 + 100 * v + 10 * M + T, M, 1 << v)
                terms = S.structure(M, T, seed=v + M + T)
                cases.append((fs, terms, None))
                if v in (1, 4, 10) and T == 3:
                    cases.append((fs, terms, O.splitmix64_field(9500 + v, v)))
    top = [np.full(1 << 10, P - 1, dtype=np.uint64)] * 3
    cases.append((top, [(P - 1, (t % 3, (t + 1) % 3, (t + 2) % 3)) for t in range(8)], None))
    # every alpha kind at one term
    for alpha in (0, 1, P - 1):
        cases.append((pool(9600, 2, 1 << 5), [(alpha, (0, 1))], None))
    # the structures do hold what the docstring says
    assert any(len(set(i)) < len(i) for _, t, _ in cases for _, i in t)
    assert any({x for _, i in t for x in i} != set(range(len(f))) for f, t, _ in cases)
    path = tmp_path / "instances.txt"
    path.write_text("\n".join(_line(*c) for c in cases) + "\n")
    lines = _run(driver, "prove", str(path)).split("\n")[:-1]
    assert len(lines) == 3 * len(cases)
    for i, (fs, terms, ch) in enumerate(cases):
        d, v, M = S.degree(terms), len(fs[0]).bit_length() - 1, len(fs)
        ref = S.prove(fs, terms, ch)
        for which, line in zip(("tail", "sums"), lines[3 * i: 3 * i + 2]):
            w = [int(x) for x in line.split()]
            assert len(w) == 2 + (d + 1) * v + v + M
            got = (w[0], w[2: 2 + (d + 1) * v], w[2 + (d + 1) * v: 2 + (d + 2) * v], w[2 + (d + 2) * v:], w[1])
            assert S.same(got, ref), (which, i, M, len(terms), v, ch is not None)
        if ch is None:
            assert lines[3 * i + 2] == "1 0 0", (i, lines[3 * i + 2])


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
            f"pool0_1_{s}": (INVALID, 1, 0), f"pool9_2_{s}": (INVALID, 2, 0), f"terms0_0_{s}": (INVALID, 0, 0),
            f"terms9_1_{s}": (INVALID, 1, 0), f"degree0_0_{s}": (INVALID, 0, 0), f"degree4_2_{s}": (INVALID, 2, 0),
            f"index2_0_{s}": (INVALID, 0, 0), f"index3_1_{s}": (INVALID, 1, 0),
            f"null_table_1_{s}": (INVALID, 1, 0), f"null_table_2_{s}": (INVALID, 2, 0),
            f"n0_0_{s}": (EMPTY, 0, 0), f"n1_1_{s}": (NO_VARIABLES, 1, 0), f"n3_1_{s}": (NOT_POW2, 1, 0),
            f"n12_2_{s}": (NOT_POW2, 2, 0), f"n2p31_2_{s}": (INVALID, 2, 0),
            f"challenge_1_{s}": (NOT_CANONICAL, 1, 0), f"challenge_p_minus_1_{s}": (OK, -1, w), f"coeff_1_{s}": (NOT_CANONICAL, 1, 0),
            f"index3_1_before_n3_1_{s}": (INVALID, 1, 0), f"n3_1_before_coeff_1_{s}": (NOT_POW2, 1, 0),
            f"coeff_0_before_pool0_1_{s}": (NOT_CANONICAL, 0, 0),
            f"no_n_tables_{s}": (INVALID, -1, 0), f"no_ns_{s}": (INVALID, -1, 0), f"no_n_terms_{s}": (INVALID, -1, 0),
            f"no_degrees_{s}": (INVALID, -1, 0), f"no_term_tables_{s}": (INVALID, -1, 0), f"no_coeffs_{s}": (INVALID, -1, 0),
            f"no_claimed_{s}": (INVALID, -1, 0), f"no_rounds_{s}": (INVALID, -1, 0), f"no_points_{s}": (INVALID, -1, 0),
            f"no_table_evals_{s}": (INVALID, -1, 0), f"no_finals_{s}": (INVALID, -1, 0),
        })
    expect.update({
        "misaligned_1_dev": (INVALID, 1, 0), "value_1_host": (NOT_CANONICAL, 1, 0),
        # the calls in order would have stopped at the table with the value >= p: it is reported, not the later shape
        "value_0_before_n12_2_host": (NOT_CANONICAL, 0, 0), "n3_1_before_value_2_host": (NOT_POW2, 1, 0),
        "value_past_the_table_host": (OK, -1, 1),
    })
    assert got == expect, {k: (got.get(k), expect.get(k)) for k in set(got) | set(expect) if got.get(k) != expect.get(k)}


def test_sop_pass_kernels_use_no_scratch_and_move_16_bytes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    asm = isa_counts.assembly(sources=("sumcheck_sop.hip",))
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)]
    assert len(names) == 4 and len(scratch) == 4 and len(lds) == 4, names  # k_sop_sums, k_sop_bind, k_sop_finish, k_sop_tails
    counts = isa_counts.count(asm)
    for k in ("k_sop_sums", "k_sop_bind"):
        i = next(j for j, n in enumerate(names) if k in n)
        print("%s: %d VGPRs, %d bytes of LDS, %d bytes of scratch" % (k, counts[k]["vgprs"], lds[i], scratch[i]))
        assert scratch[i] == 0
        assert lds[i] <= 32 * 1024
    # the pass loads and stores are 16 bytes wide: no narrower access to global memory but the partial sums' and the descriptor's
    body = {k: asm[asm.index("\n_ZN2zk10%sE" % k): asm.index(".Lfunc_end", asm.index("\n_ZN2zk10%sE" % k))] for k in ("k_sop_sums", "k_sop_bind")}
    for k, text in body.items():
        assert len(re.findall(r"global_load_dwordx4 ", text)) >= 8 * (2 if k == "k_sop_sums" else 4)
        assert not re.search(r"(global|flat)_load_(dword|dwordx2|dwordx3|ubyte|ushort) .*\bnt\b", text), k
    assert len(re.findall(r"global_store_dwordx4 ", body["k_sop_bind"])) >= 8 * 2
    assert not re.search(r"global_store_dwordx4 ", body["k_sop_sums"])
