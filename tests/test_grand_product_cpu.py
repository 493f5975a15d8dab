"""The batched grand-product argument without a GPU: the six entries in the header, the Zig binding, the ctypes table and the library;
the reference (grand_product_ref.py) against its own verifier; the host header (grand_product_host.hpp: layout, argument checks, the
walk through the layers, the host's layers, the verifier's replay and verdict) built with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone driver (tests/c_driver/grand_product_host.cpp) and run as a child process against the
reference; the gfx950 assembly of grand_product.hip (no scratch, no atomics in the layer pass, 16-byte accesses)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import exact_ref
import grand_product_ref as G
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")
P = O.P_BB
ENTRIES = {"zigz_dev_product_layers_batch": 6, "zigz_product_layers_batch": 6, "zigz_dev_grand_product_prove_batch": 13,
           "zigz_grand_product_prove_batch": 13, "zigz_dev_grand_product_verify_batch": 15, "zigz_grand_product_verify_batch": 15}
OK, EMPTY, NOT_POW2, NO_VARIABLES, NOT_CANONICAL, INVALID = 0, 1, 2, 5, 102, 103


def test_entries_in_header_binding_ctypes_and_library():
    hdr = open(os.path.join(ROOT, "include", "zigz_hip.h")).read()
    zig = open(os.path.join(ROOT, "bindings", "zig", "zigz_hip.zig")).read()
    for name, arity in ENTRIES.items():
        m = re.search(r"\b%s\(([^;]*)\);" % name, hdr)
        assert m and m.group(1).count(",") + 1 == arity, name
        z = re.search(r'pub extern "c" fn %s\(([^;]*)\) ' % name, zig)
        assert z and z.group(1).count(":") == arity, name
    assert re.search(r"#define ZIGZ_GRAND_PRODUCT_LEAF_DEFERRED 1u\b", hdr) and re.search(r"#define ZIGZ_ABI_VERSION 1\b", hdr)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name, arity in ENTRIES.items():
        assert name in _ffi.SIGNATURES and len(_ffi.SIGNATURES[name][1]) == arity
    assert _ffi.lib.zigz_abi_version() == 1 and hip.GRAND_PRODUCT_LEAF_DEFERRED == 1
    for m in ("product_layers_batch", "dev_product_layers_batch", "grand_product_prove_batch", "dev_grand_product_prove_batch",
              "grand_product_verify_batch", "dev_grand_product_verify_batch"):
        assert callable(getattr(hip.Context, m))


@pytest.mark.parametrize("v", [1, 2, 5, 9])
def test_reference_closes_and_its_verifier_accepts(v):
    """the honest chain closes at every layer (asserted inside the reference), the leaf claim is the column's extension at the leaf
    point, the tree buffer holds the numpy reduction, and fixed challenges give the same shape of proof"""
    col = G.column("random", v, seed=v)
    proof = G.prove(col)
    assert len(proof[1]) == 2 * v and len(proof[2]) == 2 * v * (v - 1) and len(proof[3]) == v * (v - 1) // 2
    assert int(proof[6]) == exact_ref.eval(col, [int(x) for x in proof[5]])
    prod = 1
    for x in col:
        prod = prod * int(x) % P
    buf = G.tree_buffer(col, fill=77)
    assert proof[0] == prod == int(buf[len(col) - 2]) and int(buf[-1]) == 77
    assert G.verdict(col, proof) == (True, int(proof[6]), int(proof[6]))
    assert G.verdict(col, proof, leaf_deferred=True) == (True, int(proof[6]), None)
    fixed = G.prove(col, G.edge_challenges(v, seed=v))
    assert [len(a) for a in fixed[1:6]] == [len(a) for a in proof[1:6]]
    assert int(fixed[6]) == exact_ref.eval(col, [int(x) for x in fixed[5]])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grand_product") / "grand_product_host")
    srcs = [os.path.join(CSRC, f) for f in ("host_hash.cpp", "host_keccak_avx512.cpp", "host_keccak_bmi.cpp",
                                            "host_keccak_avx512vl.cpp", "host_sponge_batch.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread", "-I", os.path.join(ROOT, "include"),
                           "-I", CSRC, os.path.join(ROOT, "tests", "c_driver", "grand_product_host.cpp")] + srcs + ["-o", exe])
    return exe


def _run(exe, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-3000:] + r.stderr[-6000:])
    return r.stdout


def _flat(proof):
    return ([int(proof[0]), int(proof[6])] + [int(x) for x in proof[1]] + [int(x) for x in proof[2]] + [int(x) for x in proof[3]]
            + [int(x) for x in proof[4]] + [int(x) for x in proof[5]])


@pytest.fixture(scope="module")
def cases():
    """v = 1..11 crossed with the five column kinds, Fiat-Shamir; and at every v a random and a one-zero column at fixed challenges
    drawn from 0, 1, (p + 1) / 2, p - 1 and random words"""
    out = []
    for v in range(1, 12):
        for kind in G.COLUMN_KINDS:
            out.append((G.column(kind, v, seed=v), None))
        out.append((G.column("random", v, seed=100 + v), G.edge_challenges(v, seed=v)))
        out.append((G.column("one_zero", v, seed=200 + v), G.edge_challenges(v, seed=v + 1)))
    assert {x for _, ch in out if ch is not None for x in ch} >= set(G.EDGE_WORDS)
    return out, [G.prove(c, ch) for c, ch in out]


def test_driver_proofs_and_verdicts_equal_the_reference(driver, cases, tmp_path):
    """the host prover over full trees built on the host prints the reference's proof word for word (the driver itself asserts that
    every layer's round-0 g(0) + g(1) is the carried claim and that the weight's prefix scalar ends at eq(tau, q)); the host verifier
    accepts every Fiat-Shamir proof with the reference's expected and oracle values"""
    cs, refs = cases
    path = tmp_path / "instances.txt"
    path.write_text("\n".join(" ".join(str(w) for w in [len(c), 0 if ch is None else 1] + [int(x) for x in c]
                                       + ([] if ch is None else [int(x) for x in ch])) for c, ch in cs) + "\n")
    lines = _run(driver, "prove", str(path)).split("\n")[:-1]
    at = 0
    for i, ((col, ch), ref) in enumerate(zip(cs, refs)):
        assert [int(x) for x in lines[at].split()] == _flat(ref), (i, len(col), ch is not None)
        at += 1
        if ch is None:
            want = G.verdict(col, ref)
            assert lines[at] == "%d %d %d" % (1, want[1], want[2]) and want[0], (i, lines[at])
            at += 1
    assert at == len(lines)


@pytest.mark.parametrize("v", [4, 11])
def test_host_verifier_rejects_every_tamper(driver, tmp_path, v):
    col, proof = G.pinned(v)
    t = G.tampered(col, proof)
    assert tuple(t) == G.TAMPERS

    def line(c, p):
        return " ".join(str(w) for w in [len(c)] + [int(x) for x in c] + [int(p[0])] + [int(x) for x in p[1]] + [int(x) for x in p[2]]
                        + [int(x) for x in p[5]] + [int(p[6])])

    path = tmp_path / "tampers.txt"
    path.write_text("\n".join([line(col, proof)] + [line(*t[name]) for name in G.TAMPERS]) + "\n")
    lines = _run(driver, "verify", str(path)).split("\n")[:-1]
    assert len(lines) == 2 * (1 + len(G.TAMPERS))
    assert lines[0] == "1 %d %d" % (int(proof[6]), int(proof[6])) and lines[1] == "1 %d -" % int(proof[6])
    for x, name in enumerate(G.TAMPERS):
        want = G.verdict(*t[name])
        assert not want[0]
        assert lines[2 + 2 * x] == "0 %d %d" % (want[1], want[2]), (name, lines[2 + 2 * x], want)
        deferred = G.verdict(*t[name], leaf_deferred=True)
        assert deferred[0] == (name == "column")  # without the column only the caller can notice a changed leaf
        assert lines[3 + 2 * x] == "%d %d -" % (int(deferred[0]), deferred[1]), (name, lines[3 + 2 * x])


def test_argument_checkers_and_layout(driver):
    got = {}
    for ln in _run(driver, "check").split("\n")[:-1]:
        name, st, bad = ln.split()
        got[name] = (int(st), int(bad))
    expect = {}
    for s in ("host", "dev"):
        expect.update({
            f"layers_ok_{s}": (OK, -1), f"layers_k0_{s}": (OK, -1), f"layers_k4097_{s}": (INVALID, -1), f"layers_no_out_{s}": (INVALID, -1),
            f"layers_no_ns_{s}": (INVALID, -1), f"layers_null_column_1_{s}": (INVALID, 1), f"layers_null_out_2_{s}": (INVALID, 2),
            f"layers_n0_0_{s}": (EMPTY, 0), f"layers_n1_1_{s}": (NO_VARIABLES, 1), f"layers_n12_2_{s}": (NOT_POW2, 2),
            f"layers_n2p31_2_{s}": (INVALID, 2), f"layers_null_out_0_before_n3_1_{s}": (INVALID, 0),
            f"prove_ok_{s}": (OK, -1), f"prove_ok_fixed_{s}": (OK, -1), f"prove_k0_{s}": (OK, -1), f"prove_k4097_{s}": (INVALID, -1),
            f"prove_no_products_{s}": (INVALID, -1), f"prove_no_rounds_{s}": (INVALID, -1), f"prove_no_leaf_points_{s}": (INVALID, -1),
            f"prove_null_column_2_{s}": (INVALID, 2), f"prove_n0_0_{s}": (EMPTY, 0), f"prove_n1_1_{s}": (NO_VARIABLES, 1),
            f"prove_n3_1_{s}": (NOT_POW2, 1), f"prove_n2p31_2_{s}": (INVALID, 2), f"prove_challenge_0_last_{s}": (NOT_CANONICAL, 0),
            f"prove_challenge_1_last_{s}": (NOT_CANONICAL, 1), f"prove_challenge_2_last_{s}": (NOT_CANONICAL, 2),
            f"prove_challenge_1_before_n12_2_{s}": (NOT_CANONICAL, 1), f"prove_n3_1_before_challenge_2_{s}": (NOT_POW2, 1),
            f"verify_ok_{s}": (OK, -1), f"verify_ok_deferred_{s}": (OK, -1), f"verify_deferred_with_columns_{s}": (INVALID, -1),
            f"verify_no_columns_{s}": (INVALID, -1), f"verify_flags2_{s}": (INVALID, -1), f"verify_no_n_rejected_{s}": (INVALID, -1),
            f"verify_k0_{s}": (OK, -1), f"verify_no_layer_evals_{s}": (INVALID, -1), f"verify_no_leaf_evals_{s}": (INVALID, -1),
            f"verify_n1_1_{s}": (NO_VARIABLES, 1), f"verify_deferred_n1_1_{s}": (NO_VARIABLES, 1),
            f"verify_deferred_n12_2_{s}": (NOT_POW2, 2), f"verify_product_1_{s}": (NOT_CANONICAL, 1),
            f"verify_layer_eval_0_last_{s}": (NOT_CANONICAL, 0), f"verify_layer_eval_1_last_{s}": (NOT_CANONICAL, 1),
            f"verify_round_word_0_last_{s}": (NOT_CANONICAL, 0), f"verify_round_word_1_last_{s}": (NOT_CANONICAL, 1),
            f"verify_round_word_2_last_{s}": (NOT_CANONICAL, 2), f"verify_leaf_point_1_last_{s}": (NOT_CANONICAL, 1),
            f"verify_leaf_eval_2_{s}": (NOT_CANONICAL, 2),
        })
    expect.update({
        "layers_misaligned_column_1_dev": (INVALID, 1), "layers_misaligned_out_1_dev": (INVALID, 1), "prove_misaligned_2_dev": (INVALID, 2),
        "layers_value_1_host": (NOT_CANONICAL, 1), "prove_value_2_host": (NOT_CANONICAL, 2),
        "prove_value_0_before_n3_1_host": (NOT_CANONICAL, 0), "prove_n3_1_before_value_2_host": (NOT_POW2, 1),
    })
    assert got == expect, {k: (got.get(k), expect.get(k)) for k in set(got) | set(expect) if got.get(k) != expect.get(k)}


def test_tree_kernels_use_no_scratch_and_move_16_bytes():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    asm = isa_counts.assembly(sources=("grand_product.hip",))
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)]
    lds = [int(x) for x in re.findall(r"\.group_segment_fixed_size:\s*(\d+)", asm)]
    assert len(names) == 2 and len(scratch) == 2 and len(lds) == 2, names  # k_gp_layers, k_gp_top
    counts = isa_counts.count(asm)
    for k in ("k_gp_layers", "k_gp_top"):
        i = next(j for j, n in enumerate(names) if k in n)
        print("%s: %d VGPRs, %d bytes of LDS, %d bytes of scratch" % (k, counts[k]["vgprs"], lds[i], scratch[i]))
        assert scratch[i] == 0
        assert lds[i] == (0 if k == "k_gp_layers" else 8192)
    body = asm[asm.index("\n_ZN2zk11k_gp_layersE"): asm.index(".Lfunc_end", asm.index("\n_ZN2zk11k_gp_layersE"))]
    # the three instantiations load 2 + 4 + 8 vectors and store 1 + 3 + 7, all 16 bytes wide, the loads non-temporal; no LDS and
    # no flat accesses; every vector-memory instruction of the pass is one of those loads and stores
    loads = re.findall(r"global_load_dwordx4 [^\n]*", body)
    assert len(loads) == 14 and all(re.search(r"\bnt\b", x) for x in loads), loads
    assert len(re.findall(r"global_store_dwordx4 ", body)) == 11
    assert not re.search(r"\b(ds_|flat_)", body)
    assert len(re.findall(r"\n\s+(global|buffer)_\w+ ", body)) == 14 + 11
