"""pga_plan_simplify without a GPU: what the generated graphs of tests/topo_gen.py hold (pinned on the host functions of
pangraph_amd/simplify.py, which are the expectation of the GPU tests), the ctypes mirrors against the header, simplify(topology=...) over a
pure-Python stand-in for the device call (the packing, chaining and unpacking of pangraph_amd/topology.py), and the kernels of
pga_topo_idx.h in a stand-alone program under the host sanitizers (tests/emu/topo_emu.cpp)."""
import ctypes as C
import gzip
import json
import os
import shutil
import subprocess

import pytest

import simplify_ref as sr
import topo_gen as tg
from conftest import GOLDEN, ROOT
from pangraph_amd import simplify as sp
from pangraph_amd import topology as tp

VEC = json.load(open(os.path.join(GOLDEN, "simplify_vectors.json")))
MB, CI, SR = VEC["merge_blocks"], VEC["circularize"], VEC["simplify_run"]


def _facts(lists):
    g, order, bids = tg.to_graph(*lists)
    return g, order, bids, tg.host_plan(*lists, flags=tp.COUNTS)


def _block_of(lists, name_rank):
    return sorted(b[0] for b in lists[0] if b[3])[name_rank]


# ---------------------------------------------------------------- every named case holds what it is named for
def test_wrap_cases():
    for name, dropped_first in (("wrap_dropped_at_0", True), ("wrap_anchor_at_0", False)):
        lists = tg.CASES[name]()
        g, order, bids, res = _facts(lists)
        (rnd,) = res["round"]
        first, last = lists[2][0], lists[2][2]                                  # path 1: positions 0 and 2 (its wrap)
        assert lists[1][0][3] and lists[1][0][2] == 3
        assert {first[3], last[3]} == {rnd["anchor"], rnd["other"]} and (first[3] == rnd["other"]) == dropped_first
        new_path = res["nodes"][:res["paths"][0][2]]
        assert len(new_path) == 2 and (new_path[-1][0] if dropped_first else new_path[0][0]) == res["new_nodes"][0][0]
        assert res["new_nodes"][0][1:3] == (last[1], first[2])                  # (pos0 of the pair's first node in path order, pos1 of its second)


def test_two_node_circular_has_both_edges_between_the_same_blocks():
    lists = tg.CASES["two_node_circular"]()
    _, _, _, res = _facts(lists)
    assert [t[:4] for t in res["transitive"]] == [(0, 1, 0, 0), (0, 1, 1, 1)] and len(res["round"]) == 1 and res["round"][0]["transitive"] == 0
    assert len(res["nodes"]) == 1


def test_linear_ends_do_not_pair():
    lists = tg.CASES["linear_ends"]()
    g, _, bids, res = _facts(lists)
    a, b = bids[0], bids[1]
    assert not any({bids[t[0]], bids[t[1]]} == {a, b} for t in res["edge_counts"]) and len(res["transitive"]) == 1
    circ = (lists[0], [(p[0], p[1], p[2], 1) for p in lists[1]], lists[2])
    assert any({t[0], t[1]} == {0, 1} for t in tg.host_plan(*circ)["transitive"])      # the same path closed would pair them


def test_empty_and_single_paths():
    lists = tg.CASES["empty_and_single"]()
    assert sorted(p[2] for p in lists[1]) == [0, 0, 0, 1, 1, 2] and lists[1][0][2] == 0 and lists[1][-1][2] == 0
    _, _, _, res = _facts(lists)
    assert len(res["transitive"]) == 1 and any(t[0] == t[1] for t in res["edge_counts"])       # the circular single node is a self-loop


def test_chain_takes_the_first_and_the_third_edge():
    _, _, _, res = _facts(tg.CASES["chain"]())
    assert len(res["transitive"]) == 3 and [r["transitive"] for r in res["round"]] == [0, 2]


def test_equal_lengths_anchor_is_the_smaller_id():
    lists = tg.CASES["equal_lengths"]()
    _, _, bids, res = _facts(lists)
    assert lists[0][0][1] == lists[0][1][1] and bids == [40, 900] and res["round"][0]["anchor"] == 0
    assert lists[2][0][3] == 1                                                  # the path starts in the block of the larger id


def test_one_sided_depth_is_not_transitive():
    _, _, _, res = _facts(tg.CASES["one_sided_depth"]())
    assert res["edge_counts"] == [(0, 1, 0, 0, 1)] and res["transitive"] == [] and res["nodes"] is None


def test_four_strands_in_both_orientations():
    lists = tg.CASES["four_strands"]()
    _, _, _, res = _facts(lists)
    assert sorted((t[2], t[3]) for t in res["transitive"]) == [(0, 0), (0, 1), (1, 0), (1, 1)] and all(t[4] == 2 for t in res["transitive"])
    assert len(res["round"]) == 4 and sorted(res["round"][k]["merge"][2:] for k in range(4)) == [(0, 0), (0, 0), (0, 1), (1, 0)]
    seen = set()
    for p in lists[1]:
        x, y = lists[2][p[1]], lists[2][p[1] + 1]
        seen.add((x[3] < y[3], x[5], y[5]))
    assert len(seen) == 8                                                       # every strand pair as it stands and inverted


def test_self_loop_beside_a_real_edge():
    lists = tg.CASES["self_loop"]()
    _, _, _, res = _facts(lists)
    assert (0, 0, 0, 0, 2) in res["edge_counts"] and lists[0][0][2] == 2        # the self-loop's count equals its block's depth
    assert [t[:2] for t in res["transitive"]] == [(1, 2)]


def test_reverse_anchor_is_the_right_block():
    _, _, _, res = _facts(tg.CASES["reverse_anchor"]())
    (rnd,) = res["round"]
    assert rnd["anchor_rev"] == 1 and rnd["merge"][0] == rnd["other"] and rnd["merge"][1] == rnd["anchor"] and rnd["merge"][2:] == (1, 0)
    assert res["partner"] != sorted(res["partner"]) or len(res["partner"]) == 2


def test_high_indices():
    lists = tg.CASES["high_indices"]()
    _, _, _, res = _facts(lists)
    assert min(n[3] for n in lists[2]) > 1 << 16 and res["round"] and all(t[0] > 1 << 16 for t in res["transitive"])


def test_tile_edges():
    lists, spots = tg.tile_graph()
    T, G = tg.TILE, tg.PAIR_GROUP
    assert [p[2] for p in lists[1]] == [T - 1, T, T + 1]
    _, _, _, res = _facts(lists)
    assert len(res["round"]) == len(spots) == len(res["transitive"]) == 7
    first = set(spots)
    assert T - 1 in first and 3 * T - 1 in first                                # pairs (T - 1, T) and, across the wrap, (3T - 1, 2T - 1)
    assert any((at + 1) % G == 0 and (at + 1) % T for at in first)              # a pair over the edge of a workgroup inside a tile
    got = {x[0] for x in lists[2]} - {x[0] for x in res["nodes"]}
    assert len(got) == 14 and len(res["nodes"]) == 3 * T - 7
    assert [p[1] for p in res["paths"]] == [0, T - 4, 2 * T - 6]


def test_all_but_one():
    _, _, _, res = _facts(tg.CASES["all_but_one"]())
    assert res["paths"][0][2] == 1 and res["nodes"][0][0] == res["new_nodes"][0][0]


def test_random_graphs_hold_what_the_gpu_tests_rely_on():
    n_round = n_multi = n_rev = n_wrap = n_empty = n_second = 0
    strands = set()
    for seed in range(40):
        lists = tg.random_graph(seed)
        res = tg.host_plan(*lists)
        n_round += len(res["round"]); n_multi += len(res["round"]) > 1; n_empty += not res["round"]
        n_rev += sum(r["anchor_rev"] for r in res["round"])
        strands |= {(t[2], t[3]) for t in res["transitive"]}
        for pid, off, n, circular in lists[1]:
            if circular and n > 1 and res["round"]:
                a, b = lists[2][off + n - 1], lists[2][off]
                n_wrap += any({a[3], b[3]} == {r["anchor"], r["other"]} for r in res["round"])
        nxt = tg.second_round(lists)
        n_second += bool(nxt and tg.host_plan(*nxt)["round"])
    assert n_round >= 40 and n_multi >= 10 and n_rev >= 5 and n_wrap >= 3 and n_second >= 5 and strands == {(0, 0), (0, 1), (1, 0), (1, 1)}, (n_round, n_multi, n_rev, n_wrap, n_empty, n_second, strands)


# ---------------------------------------------------------------- the C interface
def test_topo_structs_match_the_header(tmp_path):
    pairs = [("pga_topo_block_t", tp.topo_block_t), ("pga_topo_path_t", tp.topo_path_t), ("pga_topo_node_t", tp.topo_node_t), ("pga_topo_sched_t", tp.topo_sched_t),
             ("pga_topo_edge_t", tp.topo_edge_t), ("pga_topo_round_t", tp.topo_round_t), ("pga_topo_out_t", tp.topo_out_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {',
             '  printf("%d %u %u\\n", PGA_TOPO_TILE, PGA_TOPO_EDGES_ONLY, PGA_TOPO_COUNTS);']
    exp = [[str(tp.TILE), str(tp.EDGES_ONLY), str(tp.COUNTS)]]
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


def test_library_exports_the_topology_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_plan_simplify", "pga_topo_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_pack_and_unpack_are_inverse():
    for seed in range(5):
        lists = tg.random_graph(seed)
        assert tp.unpack_lists(tp.pack_lists(*lists)) == lists
        g, order, _ = tg.to_graph(*lists)
        assert tg.to_lists(g, order) == lists


# ---------------------------------------------------------------- simplify(topology=stand-in): packing, chaining, unpacking without a device
@pytest.fixture(scope="module")
def plasmids():
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    return G, [G["paths"][k]["name"] for k in sorted(G["paths"], key=int)]


def _both(graph, focal, **kw):
    t0, t1 = {}, {}
    want = sp.simplify(graph, focal, merge=sr.merge_batch, trace=t0, **kw)
    got = sp.simplify(graph, focal, merge=sr.merge_batch, trace=t1, topology=tg.host_plan, **kw)
    assert got == want and t1["rounds"] == t0["rounds"] and len(t1["transitive"]) == len(t1["rounds"])
    assert all({sp._conventional(e) for e in r} <= set(t) for r, t in zip(t1["rounds"], t1["transitive"]))
    return got, t1


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_stand_in_topology_on_the_merge_blocks_vectors(case):
    got, trace = _both(MB[case]["graph"], [None])
    assert len(trace["rounds"]) == 1 and got == sr.simplify(sr.from_json(MB[case]["graph"]), {None}, trace["rounds"])


def test_stand_in_topology_on_simplify_run_and_circularize():
    got, _ = _both(SR["graph"], SR["focal"])
    assert got == sr.from_json(SR["expected_graph"]) and set(got["nodes"]) >= {SR["NID11"], SR["NID12"]}
    _both(CI["input_graph"], [None])
    _both(CI["single_block_graph"], [None])
    # an explicit schedule, given against the conventional orientation, and a schedule that is refused
    (edge,) = sp.find_transitive_edges(sp.normalize(CI["input_graph"]))
    _both(CI["input_graph"], [None], schedule=[[sp._inv(edge)]])
    with pytest.raises((ValueError, AssertionError)):
        sp.simplify(SR["graph"], SR["focal"], schedule=[[((1, "+"), (3, "+"))]], merge=sr.merge_batch, topology=tg.host_plan)


@pytest.mark.parametrize("n_paths", [1, 3, 8])
def test_stand_in_topology_on_the_plasmids(plasmids, n_paths):
    G, names = plasmids
    got, trace = _both(G, names[:n_paths])
    assert trace["rounds"] and not sp.find_transitive_edges(got)


# ---------------------------------------------------------------- the kernels on the host
def test_topo_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_topo_idx.h: validation, every kernel, the choice of the round and the splice against a direct scalar construction; the radix sort
    and the two scans of pga_topo.hip are std::sort and plain loops here."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "topo_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "topo_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("topo_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)
