"""The host side of a commit job's build without a GPU (zigz_amd/csrc/commit_plan.hpp): the header built with AddressSanitizer +
UndefinedBehaviorSanitizer into a stand-alone driver (tests/c_driver/commit_plan_host.cpp) and run as a child process.  Checked
here: where the three builds (a commit job, a build outside a job, a batched job's arena) place the storage of the list-built
levels; that one per-proof tally gives the statistics of the two formulas zigz_commit_roots used to hold (single and batched,
restated below from that code); what a context learns about its lists' room from scripted sequences of build summaries."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zigz_amd", "csrc")

# kernels.hpp
RUN_SEG, RUN_STAGE_LEVELS, RUN_MAX_LEVELS, RUN_SUBS = 4096, 6, 20, 32
RUN_CTR_WORDS = (1 + RUN_MAX_LEVELS * RUN_SUBS) * 16 + 64
WORDS = 8 + 2 * RUN_MAX_LEVELS  # JOB_SUMMARY_WORDS
REGIONS = ["r_list", "r_stage", "bitmap", "prev", "woff", "ubase", "r_store", "g_keys", "g_idx", "g_list", "g_rep", "g_store", "upper"]
SPACES = ["WS_RUNS", "WS_RUNMETA", "WS_CONS", "WS_CONSMETA", "WS_OUT64"]
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cplan") / "commit_plan_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(ROOT, "tests", "c_driver", "commit_plan_host.cpp"), "-o", exe])
    return exe


def _run(exe, mode, lines, tmp_path):
    path = tmp_path / (mode + ".txt")
    path.write_text("".join(" ".join(str(int(x)) for x in line) + "\n" for line in lines))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, mode, str(path)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-6000:]
    return r.stdout.split("\n")[:-1]


# ---------------------------------------------------------------- the lists' functions of merkle_levels.hip / kernels.hpp, restated
def run_top_level(npad):
    return (npad - 1).bit_length() - 8


def _stage_shape(npad, l):
    s = 0 if l == 0 else (l - 1) // RUN_STAGE_LEVELS
    n_in = npad >> (s * RUN_STAGE_LEVELS)
    seg = min(n_in, RUN_SEG)
    return seg, n_in // seg, l - s * RUN_STAGE_LEVELS


def runs_lists_entries(npad, ncols, cap):
    at = 0
    for l in range(run_top_level(npad) + 1):
        seg, nseg, rel = _stage_shape(npad, l)
        worst = (ncols * nseg + RUN_SUBS - 1) // RUN_SUBS * (seg >> rel)
        at += (cap if cap and cap < worst else worst) * RUN_SUBS
    return at


def cons_lists_entries(npad, cap):
    at = 0
    for l in range(run_top_level(npad) + 1):
        worst = ((npad >> l) + RUN_SUBS - 1) // RUN_SUBS + 64
        at += (cap if cap and cap < worst else worst) * RUN_SUBS
    return at


def runs_units(npad, ncols):
    return sum(ncols * _stage_shape(npad, l)[1] for l in range(run_top_level(npad) + 1))


def runs_stage_scratch_bytes(npad, ncols):
    b, s = 64, 1
    while s * RUN_STAGE_LEVELS < run_top_level(npad):
        n = npad >> (s * RUN_STAGE_LEVELS)
        b += ncols * n * 4 + ncols * ((n + 63) // 64) * 8
        s += 1
    return b


def runs_meta_words(npad, ncols):
    return ncols * (2 * npad // 64)


def _a(x, n):
    return (x + n - 1) // n * n


def parent_totals(npad, rn, gn, ncols, r_ent, g_ent, meta, units, stage):
    """bytes of every workspace as build_trees and job_build_batch_arena sized them before they shared one layout"""
    upper = ncols * 512 * 32
    r_scratch = _a(r_ent * 4, 64) + stage + 64
    r_kept = meta * 12 + units * 4 + 64 + r_ent * 32 + 64
    g_scratch = 2 * npad * 8 + 2 * npad * 4 + _a(g_ent * 4, 64) + 64
    g_kept = 2 * npad * 4 + g_ent * gn * 32 + 64
    job = [r_scratch if rn else 0, r_kept + upper if rn else 0, g_scratch if gn else 0, (g_kept + (0 if rn else upper)) if gn else 0, 0]
    other = [_a(r_scratch, 64) + r_kept if rn else 0, 0, _a(g_scratch, 64) + g_kept if gn else 0, 0, upper]
    arena = _a(ncols * npad * 4, 256) + 2 * _a(RUN_CTR_WORDS * 8, 256)
    if rn:
        arena += sum(_a(b, 256) for b in (r_ent * 4, stage + 64, meta * 8, meta * 2, meta * 2, units * 4 + 64, r_ent * 32))
    if gn:
        arena += sum(_a(b, 256) for b in (2 * npad * 8, 2 * npad * 4, g_ent * 4, 2 * npad * 4, g_ent * gn * 32))
    return job, other, arena + _a(upper, 256)  # (the arena without its slabs, which lie behind the lists' storage now)


def parent_min_bytes(npad, rn, gn, ncols, r_ent, g_ent, meta, units, stage):
    """the least room either build gave each region"""
    r = [r_ent * 4, stage + 64, meta * 8, meta * 2, meta * 2, units * 4, r_ent * 32] if rn else [0] * 7
    g = [2 * npad * 8, 2 * npad * 4, g_ent * 4, 2 * npad * 4, g_ent * gn * 32] if gn else [0] * 5
    return r + g + [ncols * 512 * 32]


def test_layouts_are_disjoint_aligned_and_no_larger_than_before(driver, tmp_path):
    shapes = []
    for nv in (15, 16, 20, 25):
        for rn, gn in ((33, 10), (43, 0), (0, 10), (1, 1)):
            for cap in (256, 0):  # learnt (256 per sub-list) and the worst case
                npad = 1 << nv
                shapes.append((npad, rn, gn, rn + gn, runs_lists_entries(npad, rn, cap) if rn else 0, cons_lists_entries(npad, cap) if gn else 0,
                               runs_meta_words(npad, rn), runs_units(npad, rn), runs_stage_scratch_bytes(npad, rn)))
    head = lambda s: _a(s[3] * s[0] * 4, 256) + 2 * _a(RUN_CTR_WORDS * 8, 256)
    out = _run(driver, "layout", [s + (head(s),) for s in shapes], tmp_path)
    assert len(out) == 3 * len(shapes)
    for i, s in enumerate(shapes):
        npad, rn, gn = s[:3]
        want_job, want_other, want_arena = parent_totals(*s)
        least = parent_min_bytes(*s)
        for line, align, want in zip(out[3 * i:3 * i + 3], (64, 64, 256), (want_job, want_other, [want_arena, 0, 0, 0, 0])):
            name, rest = line.split(" ", 1)
            regs, totals = rest.split(" | ")
            regs = [tuple(int(x) for x in r.split(":")) for r in regs.split()]
            totals = [int(x) for x in totals.split()]
            assert len(regs) == len(REGIONS) and len(totals) == len(SPACES)
            used = [(sp, off, b, REGIONS[k]) for k, (sp, off, b) in enumerate(regs) if b]
            assert {r[3] for r in used} == {n for k, n in enumerate(REGIONS) if (k < 7 and rn) or (7 <= k < 12 and gn) or k == 12}, (s, name)
            for k, (sp, off, b) in enumerate(regs):
                assert least[k] <= b <= least[k] + (64 if least[k] else 0), (s, name, REGIONS[k])  # (at most the single build's 64 bytes of slack)
            for sp, off, b, rname in used:
                assert off % align == 0 and off + b <= totals[sp], (s, name, rname)
                if name == "arena":
                    assert sp == 0 and off >= head(s), (s, name, rname)
            for sp in range(len(SPACES)):
                here = sorted((off, off + b, rname) for sp_, off, b, rname in used if sp_ == sp)
                for (a0, a1, an), (b0, b1, bn) in zip(here, here[1:]):
                    assert a1 <= b0, (s, name, an, bn)
                assert totals[sp] <= want[sp] + 256 * len(here), (s, name, SPACES[sp], totals[sp], want[sp])
                assert (totals[sp] != 0) == (want[sp] != 0) or name == "arena", (s, name, SPACES[sp])
            where = {rname: sp for sp, off, b, rname in used}
            if gn:  # the content-addressing table is the first thing of its workspace (the generation logic compares the pointers)
                assert name == "arena" or (where["g_keys"], regs[7][1]) == (2, 0), (s, name)
            if name == "job":  # scratch apart from what the openings read; the upper levels with the R columns' (else the group's)
                assert {where.get(n, 0) for n in REGIONS[:2]} == {0} and {where.get(n, 1) for n in REGIONS[2:7]} == {1}
                assert {where.get(n, 2) for n in REGIONS[7:10]} == {2} and {where.get(n, 3) for n in REGIONS[10:12]} == {3}
                assert where["upper"] == (1 if rn else 3)
            if name == "other":
                assert {where.get(n, 0) for n in REGIONS[:7]} == {0} and {where.get(n, 2) for n in REGIONS[7:12]} == {2} and where["upper"] == 4


# ---------------------------------------------------------------- the two stats formulas zigz_commit_roots held, restated
FIELDS = ["run_aware_columns", "run_aware_dense_nodes", "run_aware_hashed", "small_domain_columns", "small_domain_fallback_waves", "cons_columns",
          "cons_dense_nodes", "cons_hashed", "cons_probe_distinct", "list_hash_perms", "keccak_permutations", "eval_constant_columns"]


def stats_single(h, f):
    run_cols, run_dense, sd_cols, cons_hinted, cons_levels_nodes, cons_sd, perms0, N = f
    st = dict(run_aware_columns=run_cols, run_aware_dense_nodes=run_dense, small_domain_columns=sd_cols, keccak_permutations=perms0)
    st["run_aware_hashed"] = h[0] if run_cols else 0
    st["eval_constant_columns"] = h[7] if run_cols else 0
    st["keccak_permutations"] -= st["run_aware_dense_nodes"] - st["run_aware_hashed"]
    st["small_domain_fallback_waves"] = h[1] if sd_cols else 0
    st["list_hash_perms"] = st["run_aware_hashed"]
    st["cons_columns"] = st["cons_dense_nodes"] = st["cons_hashed"] = st["cons_probe_distinct"] = 0
    if cons_hinted:
        st["cons_probe_distinct"] = h[5]
        if not h[4]:
            st["cons_columns"] = cons_hinted
            st["cons_dense_nodes"] = cons_hinted * cons_levels_nodes
            st["cons_hashed"] = h[3]
            st["keccak_permutations"] -= st["cons_dense_nodes"] - st["cons_hashed"]
            st["list_hash_perms"] += st["cons_hashed"]
        else:
            st["small_domain_columns"] += cons_sd
            st["keccak_permutations"] -= cons_sd * (N + N // 2)
            st["small_domain_fallback_waves"] += h[2]
            st["list_hash_perms"] += cons_hinted * cons_levels_nodes - cons_sd * (N + N // 2)
    return st


def stats_batched(hs, f):
    run_cols, run_dense, sd_cols, cons_hinted, cons_levels_nodes, cons_sd, perms0, N = f
    nz = len(hs)
    r_hashed = g_hashed = g_kept = g_distinct = constant = dense_g = 0
    for h in hs:
        r_hashed += h[0] if run_cols else 0
        constant += h[7] if run_cols else 0
        if cons_hinted:
            g_distinct += h[5]
            if not h[4]:
                g_kept += 1
                g_hashed += h[3]
            else:
                dense_g += cons_hinted * cons_levels_nodes
    st = dict(run_aware_columns=run_cols, run_aware_dense_nodes=run_dense * nz, run_aware_hashed=r_hashed, small_domain_columns=0, small_domain_fallback_waves=0,
              cons_columns=cons_hinted if g_kept else 0, cons_dense_nodes=cons_hinted * cons_levels_nodes * g_kept, cons_hashed=g_hashed,
              cons_probe_distinct=g_distinct, list_hash_perms=r_hashed + g_hashed + dense_g, eval_constant_columns=constant)
    st["keccak_permutations"] = perms0 * nz - (run_dense * nz - r_hashed) - (st["cons_dense_nodes"] - g_hashed)
    return st


def test_one_tally_gives_both_formulas(driver, tmp_path):
    rng = np.random.default_rng(20)
    cases = []
    for i in range(240):
        arena = i % 2 == 1
        nz = [1, 2, 5][(i // 2) % 3] if arena else 1
        nv = int(rng.integers(15, 21))
        N = 1 << nv
        level_nodes = sum(N >> l for l in range(nv - 8 + 1))
        run_cols = 0 if i % 7 == 0 else int(rng.integers(1, 34))
        cons_hinted = 0 if i % 5 == 0 else int(rng.integers(1, 11))
        cons_sd = 0 if arena else [0, cons_hinted, int(rng.integers(0, cons_hinted + 1))][i % 3]
        sd_cols = 0 if arena else int(rng.integers(0, 9))
        ncols = run_cols + cons_hinted + sd_cols + int(rng.integers(0, 3))
        f = (run_cols, run_cols * level_nodes, sd_cols, cons_hinted, level_nodes, cons_sd, ncols * (2 * N - 1) - sd_cols * (N + N // 2), N)
        hs = []
        for z in range(nz):
            h = [int(x) for x in rng.integers(0, 1 << 20, WORDS)]
            h[0] = int(rng.integers(0, 33 * level_nodes + 1)) if not run_cols else int(rng.integers(0, f[1] + 1))  # (ignored without R columns)
            h[3] = int(rng.integers(0, 10 * level_nodes + 1)) if not cons_hinted else int(rng.integers(0, cons_hinted * level_nodes + 1))
            h[4] = [0, 1, int(rng.integers(2, 1 << 30))][(i + z) % 3]  # kept, dropped (any value != 0)
            h[7] = int(rng.integers(0, max(run_cols, 1) + 1))
            if arena:
                h[1] = h[2] = 0  # an arena build has no small-domain counters: the summary kernel writes 0 for them
            hs.append(h)
        cases.append((nz, f, hs, arena))
    assert {c[0] for c in cases} == {1, 2, 5}
    assert any(c[1][0] == 0 for c in cases) and any(c[1][3] == 0 for c in cases)
    assert any(c[1][3] and c[1][5] == c[1][3] for c in cases) and any(c[1][3] and 0 < c[1][5] < c[1][3] for c in cases)
    assert any(len({bool(h[4]) for h in c[2]}) == 2 for c in cases)  # kept and dropped groups in one batch
    out = _run(driver, "tally", [[nz, *f] + [w for h in hs for w in h] for nz, f, hs, _ in cases], tmp_path)
    assert len(out) == len(cases)
    for line, (nz, f, hs, arena) in zip(out, cases):
        got = dict(zip(FIELDS, (int(x) for x in line.split())))
        want = stats_batched(hs, f) if arena else stats_single(hs[0], f)
        assert got == {k: v & M64 for k, v in want.items()}, (nz, f, arena, {k: (got[k], want[k]) for k in FIELDS if got[k] != want[k] & M64})


# ---------------------------------------------------------------- capacity learning: scripted summaries, results derived by hand
NPAD, TOP = 1 << 15, 7                       # levels 0 .. 7 are list-built
FACTS = (33, 0, 0, 10, 0, 0, 0, NPAD)        # 33 run-aware columns, a group of 10 (the other facts are not read)


def _summary(ru, gu, r_over=0, g_over=0, g_noslab=0, dropped=0):
    h = [0] * WORDS
    h[4] = dropped
    h[6] = r_over | (g_over << 8) | (g_noslab << 9)
    h[8:8 + TOP + 1] = ru
    h[8 + RUN_MAX_LEVELS:8 + RUN_MAX_LEVELS + TOP + 1] = gu
    return list(FACTS) + h


def _caps(r=256, g=256, npad=NPAD, g_slabs=0, g_drops=0, g_skip=0, g_kept=0, last_dropped=0):
    pad = [0] * (RUN_MAX_LEVELS - TOP - 1)
    return [npad] + [r] * (TOP + 1) + pad + [g] * (TOP + 1) + pad + [g_slabs, g_drops, g_skip, g_kept, last_dropped]


def _learn(driver, tmp_path, caps, steps):
    got = []
    for line in _run(driver, "learn", [caps] + steps, tmp_path):
        v = [int(x) for x in line.split()]
        L = RUN_MAX_LEVELS
        assert v[1 + TOP + 1:1 + L] == [0] * (L - TOP - 1) and v[1 + L + TOP + 1:1 + 2 * L] == [0] * (L - TOP - 1)  # levels above the top: untouched
        got.append(dict(again=v[0], r=v[1:1 + TOP + 1], g=v[1 + L:1 + L + TOP + 1], r_last=v[1 + 2 * L:1 + 2 * L + TOP + 1],
                        g_last=v[1 + 3 * L:1 + 3 * L + TOP + 1], g_slabs=v[-5], g_drops=v[-4], g_skip=v[-3], g_kept=v[-2], last_dropped=v[-1]))
    return got


def test_learning_fits_and_grows_before_it_runs_out(driver, tmp_path):
    # nothing ran out: a level grows only when more than 80 % of its room was used (210 * 10 > 256 * 8 -> 210 + 210 / 4 + 64 = 326,
    # 204 * 10 = 2040 is not); an empty list is remembered as 1 (0 means "no build yet")
    g, = _learn(driver, tmp_path, _caps(), [_summary([100, 210, 204, 100, 100, 100, 100, 0], [50, 50, 50, 50, 205, 50, 50, 0])])
    assert g == dict(again=0, r=[256, 326, 256, 256, 256, 256, 256, 256], g=[256, 256, 256, 256, 205 + 51 + 64, 256, 256, 256],
                     r_last=[100, 210, 204, 100, 100, 100, 100, 1], g_last=[50, 50, 50, 50, 205, 50, 50, 1],
                     g_slabs=0, g_drops=0, g_skip=0, g_kept=1, last_dropped=0)
    # caps of another shape learn nothing and never ask for a second build
    g, = _learn(driver, tmp_path, _caps(npad=1 << 16, g_kept=1), [_summary([900] * 8, [900] * 8, r_over=1, g_over=1)])
    assert g == dict(again=0, r=[256] * 8, g=[256] * 8, r_last=[0] * 8, g_last=[0] * 8, g_slabs=0, g_drops=0, g_skip=0, g_kept=1, last_dropped=0)


def test_learning_when_the_r_list_overflows(driver, tmp_path):
    # a list ran out: only the levels that needed MORE than they had grow (300 -> 300 + 75 + 64 = 439; 256 and 250 fitted), and the
    # build is repeated
    g, = _learn(driver, tmp_path, _caps(), [_summary([300, 256, 250, 10, 10, 10, 10, 10], [50] * 8, r_over=1)])
    assert g == dict(again=1, r=[439, 256, 256, 256, 256, 256, 256, 256], g=[256] * 8, r_last=[300, 256, 250, 10, 10, 10, 10, 10],
                     g_last=[50] * 8, g_slabs=0, g_drops=0, g_skip=0, g_kept=1, last_dropped=0)


def test_learning_when_a_g_list_overflows(driver, tmp_path):
    # level 1 needed 400 -> 400 + 100 + 64 = 564, and every level above gets at least the room of the one below (what they counted
    # is not to be trusted); level 0 fitted and stays
    g, = _learn(driver, tmp_path, _caps(), [_summary([10] * 8, [100, 400, 120, 50, 50, 50, 50, 50], g_over=1)])
    assert g == dict(again=1, r=[256] * 8, g=[256, 564, 564, 564, 564, 564, 564, 564], r_last=[10] * 8,
                     g_last=[100, 400, 120, 50, 50, 50, 50, 50], g_slabs=0, g_drops=0, g_skip=0, g_kept=1, last_dropped=0)
    # ... but not when the group was dropped anyway: nothing to learn from its lists, no second build for them
    g, = _learn(driver, tmp_path, _caps(g_slabs=1), [_summary([10] * 8, [100, 400, 120, 50, 50, 50, 50, 50], g_over=1, dropped=1)])
    assert g == dict(again=0, r=[256] * 8, g=[256] * 8, r_last=[10] * 8, g_last=[0] * 8, g_slabs=1, g_drops=1, g_skip=0, g_kept=0, last_dropped=1)


def test_learning_drops_skips_and_keeps(driver, tmp_path):
    drop_noslab = _summary([10] * 8, [0] * 8, g_noslab=1, dropped=1)
    drop = _summary([10] * 8, [0] * 8, dropped=7)
    keep = _summary([10] * 8, [20] * 8)
    got = _learn(driver, tmp_path, _caps(g_kept=5), [drop_noslab] + [drop] * 9 + [keep, keep])
    # dropped with nowhere to build the columns densely: build again, with slabs from now on
    assert got[0] == dict(again=1, r=[256] * 8, g=[256] * 8, r_last=[10] * 8, g_last=[0] * 8, g_slabs=1, g_drops=1, g_skip=0, g_kept=0, last_dropped=1)
    # that second build is the second drop in a row: skip 15 jobs, twice as many after every further drop, at most 15 << 6
    assert [g["g_skip"] for g in got[1:10]] == [15, 30, 60, 120, 240, 480, 960, 960, 960]
    assert [g["g_drops"] for g in got[1:10]] == list(range(2, 11))
    assert all(g["again"] == 0 and g["g_slabs"] == 1 and g["g_kept"] == 0 and g["last_dropped"] == 1 for g in got[1:10])
    # kept twice (the count build_trees leaves the probe pass out from); what is left to skip is counted down by the builds, not here
    assert [(g["g_kept"], g["g_drops"], g["g_skip"], g["last_dropped"], g["g_slabs"], g["again"]) for g in got[10:]] == \
        [(1, 0, 960, 0, 1, 0), (2, 0, 960, 0, 1, 0)]
    assert got[11]["g_last"] == [20] * 8 and got[11]["g"] == [256] * 8
