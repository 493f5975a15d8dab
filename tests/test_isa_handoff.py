"""Hand-offs to the host through pinned memory, checked in the gfx950 assembly (CPU only: hipcc cross-compiles).

A kernel that publishes results into pinned host memory ends with: every thread fences its stores system-wide
(`buffer_wbl2 sc0 sc1`), then one thread counts its workgroup with a returning atomic (`global_atomic_add ... sc0`), and the
workgroup that completes the count stores the completion word the host polls for.  With more than one wave per workgroup
the count must wait behind an `s_barrier`: otherwise thread 0 of wave 0 can count the workgroup while waves 1.. have not
yet fenced (or even issued) their stores, and the host reads stale words once it sees the completion word."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ("kernels.hip", "merkle_levels.hip", "sumcheck_batch.hip")
# kernels known to publish this way with more than one wave per workgroup (a rename must not make the check vacuous)
KNOWN_PUBLISHERS = {"k_publish<4>", "k_publish<8>", "k_batch_publish", "k_batch_tails", "k_radix_finalize"}

_ATOMIC = re.compile(r"^global_atomic_add\w*\s.*\bsc0\b")


def _functions(asm):
    """{mangled name: [instruction lines]} of every function body"""
    out, cur = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            cur = None
        elif t and not t.startswith((".", ";")) and not t.endswith(":"):
            out[cur].append(t)
    return out


def _max_workgroup(asm):
    """{mangled kernel name: .max_flat_workgroup_size} from the code object metadata"""
    out = {}
    meta = asm.split("amdhsa.kernels:")
    for doc in meta[1:]:
        for item in re.split(r"\n  - ", doc):
            size = re.search(r"\.max_flat_workgroup_size:\s*(\d+)", item)
            name = re.search(r"\n\s+\.name:\s+(\S+)", item)
            if size and name:
                out[name.group(1)] = int(size.group(1))
    return out


def _pretty(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return {n: re.sub(r"\(.*$", "", p).replace("void ", "").replace("zk::", "") for n, p in zip(names, r)}


def handoffs(asm):
    """[(kernel, max workgroup size, barrier between fence and count)] for every returning atomic add that follows a
    system-wide release fence, in kernels of more than one wave"""
    funcs, wg = _functions(asm), _max_workgroup(asm)
    names = _pretty(list(funcs))
    found = []
    for mangled, body in funcs.items():
        size = wg.get(mangled, 0)
        if size <= 64:
            continue
        fence, barrier = None, False
        for ins in body:
            if ins.startswith("buffer_wbl2"):
                fence, barrier = ins, False
            elif ins.startswith("s_barrier"):
                barrier = True
            elif _ATOMIC.match(ins) and fence is not None:
                found.append((names[mangled], size, barrier))
    return found


def test_multi_wave_publishers_count_behind_a_barrier():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_counts
    asm = isa_counts.assembly(sources=SOURCES)
    found = handoffs(asm)
    kernels = {k for k, _, _ in found}
    assert KNOWN_PUBLISHERS <= kernels, f"the rule no longer finds {sorted(KNOWN_PUBLISHERS - kernels)}"
    racy = sorted({f"{k} ({size} threads)" for k, size, barrier in found if not barrier})
    assert not racy, "fence -> count without s_barrier in multi-wave kernels: " + ", ".join(racy)


def test_the_rule_sees_a_missing_barrier():
    """the scan itself: the same fence/count sequence with and without the barrier, in a 256-thread kernel"""
    body = ["buffer_wbl2 sc0 sc1", "s_waitcnt vmcnt(0)", "{}", "v_mov_b32 v1, 1", "global_atomic_add v1, v1, v2, s[4:5] sc0",
            "s_endpgm"]

    def asm(with_barrier, size):
        lines = [b if b != "{}" else ("s_barrier" if with_barrier else "s_nop 0") for b in body]
        return ("_ZN2zk5k_fooEv:\n\t" + "\n\t".join(lines) + "\n.Lfunc_end0:\n"
                "amdhsa.kernels:\n  - .agpr_count: 0\n    .max_flat_workgroup_size: %d\n    .name:           _ZN2zk5k_fooEv\n" % size)

    assert handoffs(asm(True, 256)) == [("k_foo", 256, True)]
    assert handoffs(asm(False, 256)) == [("k_foo", 256, False)]
    assert handoffs(asm(False, 64)) == []  # one wave: the cheap form is enough
