"""Batched Merkle commitments without a GPU: the ABI entries and the opaque handle in the header, the generated Zig binding and
the library; the host batchVerify against openings built by the oracle; and the gfx950 assembly of merkle_batch.hip (no
scratch, every multi-wave publisher counts its workgroup behind a barrier)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = O.P_BB
ENTRIES = ["zigz_dev_merkle_commit_batch", "zigz_merkle_commit_batch", "zigz_merkle_open_batch", "zigz_commit_open_batch",
           "zigz_merkle_batch_destroy"]


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_entries_in_header_binding_and_library():
    hdr = _read("include", "zigz_hip.h")
    zig = _read("bindings", "zig", "zigz_hip.zig")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert f'pub extern "c" fn {name}(' in zig, name
    assert "typedef struct zigz_merkle_batch zigz_merkle_batch;" in hdr
    assert "pub const MerkleBatch = opaque {};" in zig
    assert zig.count("extern struct") == 9  # the handle is opaque: no new value struct
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi
    for name in ENTRIES:
        assert name in _ffi.SIGNATURES


def _openings(seed, logs):
    rng = np.random.default_rng(seed)
    commitments, proofs = [], []
    for j, v in enumerate(logs):
        ev = O.splitmix64_field(seed * 100 + j, 1 << v)
        pt = [int(x) for x in rng.integers(0, P, size=v)]
        val, idx, sib, dirs, leaf = O.commit_open(P, ev, pt)
        commitments.append((O.merkle_build(ev)[0], v))
        proofs.append(dict(point=pt, value=val, index=idx, leaf=leaf, siblings=sib, directions=dirs))
    return commitments, proofs


def test_host_batch_verify_accepts_oracle_openings_and_rejects_tampering():
    from zigz_amd import host
    commitments, proofs = _openings(3, [0, 1, 4, 7, 10])
    assert host.batch_verify(commitments, proofs)
    assert host.batch_verify([], [])
    assert not host.batch_verify(commitments, proofs[:-1])
    for i, (_, v) in enumerate(commitments):
        bad = [dict(p) for p in proofs]
        bad[i]["leaf"] = (proofs[i]["leaf"] + 1) % P
        assert not host.batch_verify(commitments, bad), ("leaf", i)
        if v == 0:
            continue
        for l in (0, v - 1):
            s = bytearray(proofs[i]["siblings"])
            s[32 * l + 5] ^= 1
            bad = [dict(p) for p in proofs]
            bad[i]["siblings"] = bytes(s)
            assert not host.batch_verify(commitments, bad), ("sibling", i, l)
            d = bytearray(proofs[i]["directions"])
            d[l] ^= 1
            bad = [dict(p) for p in proofs]
            bad[i]["directions"] = bytes(d)
            assert not host.batch_verify(commitments, bad), ("direction", i, l)
        bad = [dict(p) for p in proofs]
        bad[i]["point"] = proofs[i]["point"][:-1]  # num_vars mismatch (polynomial_commit.zig:123-125)
        assert not host.batch_verify(commitments, bad), ("point", i)


@pytest.fixture(scope="module")
def asm():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    return isa_counts.assembly(sources=("merkle_batch.hip",))


def test_merkle_batch_kernels_use_no_scratch(asm):
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    assert len(names) >= 5 and len(sizes) == len(names)
    assert all(int(s) == 0 for s in sizes), dict(zip(names, sizes))


def test_merkle_batch_publishers_count_behind_a_barrier(asm):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_isa_handoff import handoffs
    found = handoffs(asm)
    assert "k_mbatch_roots" in {k for k, _, _ in found}
    racy = sorted({f"{k} ({size} threads)" for k, size, barrier in found if not barrier})
    assert not racy, "fence -> count without s_barrier in multi-wave kernels: " + ", ".join(racy)
