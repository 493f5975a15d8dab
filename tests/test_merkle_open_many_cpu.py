"""Many openings per committed tree without a GPU: the ABI entries in the header, the generated Zig binding, the ctypes
signatures and the library; the host side (argument checks, offset prefix, chunk plan) on mixed heights; and the gfx950
assembly of the two kernels (no scratch, no LDS, full 16-byte stores -- non-temporal in the device form -- and a barrier
between the system-wide fence and the workgroup count)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["zigz_merkle_open_many", "zigz_dev_merkle_open_many", "zigz_commit_open_many"]


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


def test_entries_in_header_binding_and_library():
    hdr = _read("include", "zigz_hip.h")
    zig = _read("bindings", "zig", "zigz_hip.zig")
    for name in ENTRIES:
        assert re.search(r"\b%s\(" % name, hdr), name
        assert f'pub extern "c" fn {name}(' in zig, name
    assert zig.count("extern struct") == 9  # parallel arrays: no new value struct
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "zigz_amd", "lib", "libzigz_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert set(ENTRIES) <= syms, sorted(set(ENTRIES) - syms)
    from zigz_amd import _ffi, hip
    for name in ENTRIES:
        assert name in _ffi.SIGNATURES
    assert len(_ffi.SIGNATURES["zigz_merkle_open_many"][1]) == 11 and len(_ffi.SIGNATURES["zigz_commit_open_many"][1]) == 8
    for cls, names in ((hip.MerkleBatch, ("open_many", "dev_open_many")), (hip.CommitJob, ("open_many",))):
        for n in names:
            assert callable(getattr(cls, n))


def test_the_plan_limit_is_the_verify_entries_limit():
    hdr = _read("include", "zigz_hip.h")
    plan = _read("zigz_amd", "csrc", "open_plan.hpp")
    m = re.search(r"#define ZIGZ_VERIFY_BATCH_MAX (\d+)\b", hdr)
    assert m and int(m.group(1)) == 1 << 22
    assert "MAX_OPENINGS = (size_t)1 << 22" in plan


def test_host_checks_offsets_and_chunks_on_mixed_heights(tmp_path):
    exe = str(tmp_path / "open_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "zigz_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_driver", "open_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "open_plan: 41 case(s), 0 failure(s)" in r.stdout


def test_c_driver_calls_open_many(tmp_path):
    """tests/c_driver/open_many_driver.c compiles as C against the header and links against the library; without a GPU it
    stops at the missing device (exit 77), with one it must pass."""
    exe = str(tmp_path / "open_many_driver")
    lib = os.path.join(ROOT, "zigz_amd", "lib")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c_driver", "open_many_driver.c"), "-o", exe, "-L" + lib, "-lzigz_hip",
                           "-Wl,-rpath," + lib])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode in (0, 77), r.stdout + r.stderr
    if r.returncode == 0:
        assert "open_many_driver: ok" in r.stdout


@pytest.fixture(scope="module")
def kernels():
    """{kernel: (metadata item, body)} of k_mbatch_open_many<false / true> and k_open_many"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import isa_counts
    from test_isa_handoff import _functions, _pretty, handoffs
    out, found = {}, []
    for src in ("merkle_batch.hip", "kernels.hip"):
        asm = isa_counts.assembly(sources=(src,))
        funcs = _functions(asm)
        names = _pretty(list(funcs))
        meta = {}
        for item in re.split(r"\n  - ", asm.split("amdhsa.kernels:")[1]):
            name = re.search(r"\n\s+\.name:\s+(\S+)", item)
            if name:
                meta[name.group(1)] = item
        for mangled, body in funcs.items():
            if "open_many" in names[mangled] and mangled in meta:
                out[names[mangled]] = (meta[mangled], body)
        found += [h for h in handoffs(asm) if "open_many" in h[0]]
    return out, found


def test_open_many_kernels_use_no_scratch_and_no_lds(kernels):
    ks, _ = kernels
    assert sorted(ks) == ["k_mbatch_open_many<false>", "k_mbatch_open_many<true>", "k_open_many"], sorted(ks)
    for k, (meta, _) in ks.items():
        assert int(re.search(r"\.private_segment_fixed_size:\s*(\d+)", meta).group(1)) == 0, k
        assert int(re.search(r"\.group_segment_fixed_size:\s*(\d+)", meta).group(1)) == 0, k


def test_open_many_kernels_store_whole_16_byte_pieces(kernels):
    ks, _ = kernels
    for k, (_, body) in ks.items():
        stores = [i for i in body if i.startswith("global_store_dwordx4")]
        assert stores, k
        if k == "k_mbatch_open_many<true>":  # device outputs: kept out of the caches
            assert all(re.search(r"\bnt\b", i) for i in stores), stores
        else:
            assert not any(re.search(r"\bnt\b", i) for i in stores), stores


def test_open_many_publishers_count_behind_a_barrier(kernels):
    ks, found = kernels
    assert {k for k, _, _ in found} == set(ks)  # each of them hands off through pinned memory (the device form: a null flag)
    racy = sorted({f"{k} ({size} threads)" for k, size, barrier in found if not barrier})
    assert not racy, "fence -> count without s_barrier in multi-wave kernels: " + ", ".join(racy)
