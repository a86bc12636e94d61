"""pga_apply_merge without a GPU: what the cases of tests/apply_gen.py hold (pinned on host_apply, the host reweave() of
pangraph_amd/reweave.py, which is the expectation of the GPU tests), the ctypes mirrors against the header, reweave(update=...) over a
stand-in for the device call (the packing and the reading back of pangraph_amd/reweave.py), and the kernels of pga_apply_idx.h in a
stand-alone program under the host sanitizers (tests/emu/apply_emu.cpp)."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

import apply_gen as ag
import reweave_gen as rg
import reweave_ref as rr
import topo_gen as tg
from conftest import GOLDEN, ROOT
from pangraph_amd import apply as ap
from pangraph_amd import reweave as rw

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))


def _path(exp, k):
    _, off, n, _ = exp["paths"][k]
    return exp["nodes"][off:off + n]


# ---------------------------------------------------------------- every named case holds what it is named for
def test_reference_vector():
    c = ag.case("reference")
    exp = c["exp"]
    assert sorted(b[1] for b in exp["new_blocks"]) == [0, 0, 1, 1, 1, 1] and len(c["promises"]) == 4
    assert {c["args"][0][k[0]][0] for k in c["args"][3]} == {10, 20, 30, 40, 50} and exp["block_map"] == [ag.NONE] * 5
    w = VEC["reweave_graph"]
    assert [p[2] for p in exp["paths"]] == [w["expected_path_lengths"][str(p[0])] for p in exp["paths"]]
    assert ["".join("+-"[n[5]] for n in _path(exp, k)) for k in range(len(exp["paths"]))] == [w["expected_strands"][str(p[0])] for p in exp["paths"]]


def test_three_intervals_on_a_forward_and_a_reverse_node():
    c = ag.case("three_intervals_both_strands")
    blocks, paths, nodes, cut, ivs, slices, members = c["args"]
    assert [(n[3], n[5]) for n in nodes] == [(0, 0), (1, 0), (0, 1)] and cut == [(0, 3, 0)] and len(ivs) == 3
    exp = c["exp"]
    assert [b[0] for b in exp["blocks"]] == [2, 500, 501, 502]
    assert [n[3] for n in exp["nodes"]] == [1, 2, 3, 0, 3, 2, 1]               # the reverse node's new nodes in reversed order
    assert exp["old_node"] == [nodes[0][0], nodes[2][0]] * 3 and exp["block_map"] == [ag.NONE, 0]


def test_dropped_members_and_an_empty_path():
    c = ag.case("dropped_everywhere")
    blocks, paths, nodes = c["args"][:3]
    assert [(p[2], p[3]) for p in paths] == [(5, 0), (1, 0), (2, 1)] and [n[3] for n in nodes[:5]] == [0, 1, 0, 1, 0]
    assert [s[1:] for s in c["args"][5]] == [(1, 4), (1, 4)]
    exp = c["exp"]
    assert [(p[1], p[2]) for p in exp["paths"]] == [(0, 2), (2, 0), (2, 3)]    # first, middle and last position gone; path 2 empty
    assert [n[3] for n in exp["nodes"]] == [0, 0, 0, 1, 2]


def test_two_nodes_of_one_path_in_one_cut_block():
    c = ag.case("two_nodes_one_block")
    assert [n[3] for n in c["args"][2]] == [0, 0, 1]
    assert [n[3] for n in c["exp"]["nodes"]] == [1, 2, 2, 1, 0]


def test_cut_nodes_at_both_ends_of_a_circular_path():
    c = ag.case("circular_ends")
    assert c["args"][1] == [(1, 0, 4, 1)] and [n[3] for n in c["args"][2]] == [0, 1, 2, 0]
    assert c["exp"]["paths"] == [(1, 0, 8, 1)] and [n[3] for n in c["exp"]["nodes"]] == [2, 3, 4, 0, 1, 4, 3, 2]


@pytest.mark.parametrize("n_before", [ag.TILE - 1, ag.TILE, ag.TILE + 1])
def test_tile_edges(n_before):
    c = ag.case(f"tile_{n_before}")
    nodes, exp = c["args"][2], c["exp"]
    assert len(nodes) == n_before + 2 and [n[3] for n in nodes[n_before - 1:]] == [0, 1, 0]
    assert len(exp["nodes"]) == n_before + 6 and [n[3] for n in exp["nodes"][n_before - 1:]] == [0, 1, 2, 3, 4, 5, 0]


def test_second_level_of_the_tile_scan():
    c = ag.case("second_level")
    nodes, exp = c["args"][2], c["exp"]
    n = ag.TILE * ag.SCAN_THREADS
    assert len(nodes) > n and [i for i, x in enumerate(nodes) if x[3] == 1] == [0, n - 1, n, n + 39] and nodes[n][5] == 1
    assert len(exp["nodes"]) == len(nodes) + 4 and [x[3] for x in exp["nodes"][n:n + 4]] == [1, 2, 2, 1]


def test_forty_intervals():
    c = ag.case("forty_intervals")
    exp = c["exp"]
    assert c["args"][3] == [(0, 40, 0)] and len(exp["new_blocks"]) == 40 and len(exp["new_nodes"]) == 120
    assert [n[3] for n in _path(exp, 0)] == list(range(1, 41)) + [0] + list(range(40, 0, -1)) and [n[3] for n in _path(exp, 1)] == list(range(40, 0, -1))


def test_new_ids_below_between_and_above_the_survivors():
    c = ag.case("id_ranges")
    exp = c["exp"]
    assert [b[0] for b in exp["blocks"]] == [50, 100, 150, 199, 200, 1 << 63, (1 << 64) - 1]
    assert [b[0] for b in exp["new_blocks"]] == [0, 2, 3, 5, 6] and exp["block_map"] == [1, ag.NONE, 4]
    assert [b[2] for b in exp["new_blocks"]] == [2, 1, 4, 3, 0]                # interval_a: the table is by id, not by interval


def test_merged_block_members_interleave():
    c = ag.case("interleaved_merge")
    exp, ivs, slices = c["exp"], c["args"][4], c["args"][5]
    (merged,) = [b for b in exp["new_blocks"] if b[1] == 1]
    assert ivs[merged[2]]["is_anchor"] and not ivs[merged[3]]["is_anchor"] and exp["blocks"][merged[0]][1:3] == (20, 8)
    src = exp["member_src"][merged[4]:merged[4] + 8]
    side = [int(slices[merged[2]][0] <= k < slices[merged[2]][0] + 4) for k in src]
    assert sorted(side) == [0] * 4 + [1] * 4 and side != sorted(side) and side != sorted(side, reverse=True)
    assert [exp["new_nodes"][k][4] for k in src] == list(range(8)) and [exp["new_nodes"][k][0] for k in src] == sorted(exp["new_nodes"][k][0] for k in src)


def test_block_index_above_2_16():
    c = ag.case("high_index")
    assert c["args"][3][0][0] > 1 << 16 and min(n[3] for n in c["args"][2]) > 1 << 16
    assert c["exp"]["block_map"][:(1 << 16) + 5] == [ag.NONE] * ((1 << 16) + 5) and c["exp"]["block_map"][-2:] == [ag.NONE, 0]
    assert c["exp"]["blocks"] == ag.case("three_intervals_both_strands")["exp"]["blocks"]


def test_unaligned_slice_without_a_member():
    c = ag.case("empty_unaligned")
    exp = c["exp"]
    assert c["args"][5][1][1:] == (0, 2) and exp["blocks"][2] == (501, 10, 0, 1)
    assert [b[0] for b in exp["new_blocks"]] == [1, 2, 3] and exp["new_blocks"][1][4] == exp["new_blocks"][2][4] == 2


def test_empty_cut():
    c = ag.case("no_cut")
    assert c["args"][3:] == ([], [], [], []) and c["exp"] == {f: None if f in ("blocks", "paths", "nodes") else [] for f in ag.OUT_FIELDS}


def test_random_graphs_hold_what_the_gpu_tests_rely_on():
    n_merged = n_rev = n_circ = n_shrunk = n_high = n_surv = n_second = 0
    for seed in range(40):
        c = ag.random_case(seed)
        blocks, paths, nodes, cut, ivs, slices, members = c["args"]
        exp = c["exp"]
        gone = {k[0] for k in cut}
        n_merged += sum(b[1] for b in exp["new_blocks"])
        n_rev += sum(1 for n in nodes if n[3] in gone and n[5] and cut[[k[0] for k in cut].index(n[3])][1] > 1)
        n_circ += sum(1 for p in paths if p[3] and any(n[3] in gone for n in nodes[p[1]:p[1] + p[2]]))
        n_shrunk += sum(s[2] for s in slices)
        n_high += sum(1 for b in exp["blocks"] if b[0] >= 1 << 63)
        n_surv += sum(1 for m in exp["block_map"] if m != ag.NONE)
        nxt = ag.fresh_cut(c, seed) if seed < 12 else None
        n_second += bool(nxt and nxt["args"][3])
    assert n_merged >= 100 and n_rev >= 50 and n_circ >= 20 and n_high >= 50 and n_surv >= 20 and n_second >= 8, (n_merged, n_rev, n_circ, n_shrunk, n_high, n_surv, n_second)


def test_graphs_after_hold_transitive_edges():
    from pangraph_amd import simplify as sp
    counts = [len(sp.find_transitive_edges(c["after"])) for c in ag.simplify_cases()]
    assert sum(counts) >= 50 and sum(1 for n in counts[7:] if n) >= 3 and counts[1] == 39      # (39: the forty pieces of one block, in a row on every path)


# ---------------------------------------------------------------- the C interface
def test_apply_structs_match_the_header(tmp_path):
    pairs = [("pga_apply_cut_t", ap.apply_cut_t), ("pga_apply_block_t", ap.apply_block_t), ("pga_apply_out_t", ap.apply_out_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp


def test_library_exports_the_apply_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_apply_merge", "pga_apply_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_pack_cut_takes_the_plan_records():
    plan = {"blocks": [{"block": 2, "n_intervals": 3, "first_interval": 0}, {"block": 0, "n_intervals": 1, "first_interval": 3}]}
    n, K = ap.pack_cut(plan, [7, 8, 9])
    assert n == 2 and [(K[i].block, K[i].n_intervals, K[i].first_interval) for i in range(n)] == [(9, 3, 0), (7, 1, 3)]


def test_expected_lists_are_what_pack_graph_gives():
    for c in [ag.case(n) for n in ("reference", "interleaved_merge", "dropped_everywhere", "tile_1024")] + [ag.random_case(s) for s in range(5)]:
        for g in (c["before"], c["after"]):
            order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
            assert ag.lists_of(g, order) == tg.to_lists(g, order)
        assert ag.lists_of(c["after"], {b: sorted(blk["alignments"]) for b, blk in c["after"]["blocks"].items()}) == (c["exp"]["blocks"], c["exp"]["paths"], c["exp"]["nodes"])


# ---------------------------------------------------------------- reweave(update=stand-in): packing and reading back without a device
def test_stand_in_update_on_the_reference_vector():
    c = ag.case("reference")
    calls = []

    def stand_in(*args):
        calls.append(args)
        assert args == c["args"]
        return c["exp"]

    thr = VEC["reweave"]["thr_len"]
    g0, matches = rg.reference_graph(VEC)
    g1, _ = rg.reference_graph(VEC)
    want = rw.reweave(g0, matches, thr, plan=rr.expected_call, slicer=ag.ref_slicer)
    got = rw.reweave(g1, matches, thr, plan=rr.expected_call, slicer=ag.ref_slicer, update=stand_in)
    assert got == want and len(calls) == 1 and len(got[1]) == 4


def test_stand_in_update_on_random_graphs():
    for seed in range(6):
        c = ag.random_case(seed)
        g, matches = ag.random_graph(seed)
        want = rw.reweave(ag.random_graph(seed)[0], matches, rg.THR, plan=rr.expected_call, slicer=ag.ref_slicer)
        assert rw.reweave(g, matches, rg.THR, plan=rr.expected_call, slicer=ag.ref_slicer, update=lambda *a: c["exp"]) == want


# ---------------------------------------------------------------- the kernels on the host
def test_apply_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_apply_idx.h: validation, every kernel and the splice behind them against a direct scalar construction, and every refusal; the radix
    sorts and the scans of pga_apply.hip are std::stable_sort and plain loops here."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "apply_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "apply_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("apply_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)
