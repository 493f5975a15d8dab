"""Batched Merkle verification without a GPU: the ABI entries in the header, the generated Zig binding, the ctypes signatures
and the library; the host side (counting sort by height, chunk plan, level-major staging) on ragged height mixes; and the
gfx950 assembly of merkle_verify.hip (no scratch, system-wide fence of the verdicts, no multi-wave publisher that counts
without a barrier)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zigz_merkle_verify_batch", "zigz_dev_merkle_verify_batch"]


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_entries_in_header_binding_and_library():
    hdr = _read("include", "zigz_hip.h")
    zig = _read("bindings", "zig", "zigz_hip.zig")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert f'pub extern "c" fn {name}(' in zig, name
    assert re.search(r"#define ZIGZ_VERIFY_BATCH_MAX 4194304\b", hdr)
    assert "pub const VERIFY_BATCH_MAX = 4194304;" in zig
    assert zig.count("extern struct") == 9  # plain arrays: no new value struct
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, host
    for name in ENTRIES:
        assert name in _ffi.SIGNATURES
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_host.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "zigzh_batch_verify_dev" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert "zigzh_batch_verify_dev" in host.SIGNATURES


def test_host_bucketing_and_staging_on_ragged_heights(tmp_path):
    exe = str(tmp_path / "verify_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-pthread", "-I",
                           os.path.join(ROOT, "zigz_amd", "csrc"), os.path.join(ROOT, "tests", "c_driver", "verify_plan.cpp"),
                           "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "verify_plan: 40 case(s), 0 failure(s)" in r.stdout


@pytest.fixture(scope="module")
def asm():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    return isa_counts.assembly(sources=("merkle_verify.hip",))


def _bodies(asm):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_isa_handoff import _functions, _pretty
    funcs = _functions(asm)
    names = _pretty(list(funcs))
    return {names[m]: body for m, body in funcs.items()}


def test_merkle_verify_kernels_use_no_scratch(asm):
    sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
    names = re.findall(r"\n\s+\.name:\s+(_Z\w+)", asm)
    assert len(names) == 4 and len(sizes) == len(names)  # k_mverify<dev, pause>
    assert all(int(s) == 0 for s in sizes), dict(zip(names, sizes))


def test_merkle_verify_fences_its_verdicts_and_counts_behind_a_barrier(asm):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_isa_handoff import handoffs
    bodies = _bodies(asm)
    verify = {k: b for k, b in bodies.items() if k.startswith("k_mverify")}
    assert len(verify) == 4, sorted(bodies)
    for k, body in verify.items():
        # the verdict bytes go to pinned memory: a system-wide release fence follows the last of them
        stores = [i for i, ins in enumerate(body) if ins.startswith("global_store_byte")]
        fences = [i for i, ins in enumerate(body) if ins.startswith("buffer_wbl2")]
        assert stores and fences and max(fences) > max(stores), k
    racy = sorted({f"{k} ({size} threads)" for k, size, barrier in handoffs(asm) if not barrier})
    assert not racy, "fence -> count without s_barrier in multi-wave kernels: " + ", ".join(racy)
    # the hand-off of the reject count is k_publish<8> (kernels.hip), a known multi-wave publisher behind a barrier
    from test_isa_handoff import KNOWN_PUBLISHERS
    assert "k_publish<8>" in KNOWN_PUBLISHERS
    assert "launch_publish_u64(d_rej" in _read("zigz_amd", "csrc", "api_merkle_verify.cpp")
