"""`pangraph simplify` without a GPU: the restatement tests/simplify_ref.py against the reference's own unit-test values
(tests/golden/simplify_vectors.json), the graph level of pangraph_amd/simplify.py against the restatement (which stands in for the device
call), the plasmid fixture reduced to a few paths, the ctypes mirrors against the header, the index arithmetic of the kernels in a
stand-alone program under the host sanitizers (tests/emu/merge_emu.cpp), and what the GPU tests rely on their generated batches for."""
import copy
import gzip
import json
import os
import shutil
import subprocess

import pytest

import reconstruct_ref as rr
import simplify_gen as sg
import simplify_ref as sr
from conftest import GOLDEN, ROOT
from pangraph_amd import simplify as sp

VEC = json.load(open(os.path.join(GOLDEN, "simplify_vectors.json")))
MB, CI, SR = VEC["merge_blocks"], VEC["circularize"], VEC["simplify_run"]
PLASMID_COUNTS = (1, 3, 8)


def _edge(e):
    return tuple((b, s) for b, s in e)


def _new_ids(new_nodes):
    return {int(k): sr.node_id(n["block_id"], n["path_id"], n["strand"], n["position"]) for k, n in new_nodes.items()}


def _resolve(g, ids):
    """an expected graph whose '@k' entries stand for the id of new node k -> the restatement's shape"""
    key = lambda k: ids[int(k[1:])] if isinstance(k, str) and k.startswith("@") else int(k)
    g = copy.deepcopy(g)
    for kind in ("nodes",):
        g[kind] = {str(key(k)): v for k, v in g[kind].items()}
    for b in g["blocks"].values():
        b["alignments"] = {str(key(k)): v for k, v in b["alignments"].items()}
    for p in g["paths"].values():
        p["nodes"] = [key(n) for n in p["nodes"]]
    return sr.from_json(g)


def _block(b):
    return sr.from_json({"paths": {}, "nodes": {}, "blocks": {"0": b}})["blocks"][0]


@pytest.fixture(scope="module")
def plasmids():
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    names = [G["paths"][k]["name"] for k in sorted(G["paths"], key=int)]
    fa_names, fa_seqs = rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))
    return G, names, dict(zip(fa_names, fa_seqs))


# ---------------------------------------------------------------- the restatement against the reference's values
def test_node_id_is_the_reference_hash():
    for name, (b, p, s, pos) in SR["node_id_inputs"].items():
        assert sr.node_id(b, p, s, pos) == SR[name] == sp.node_id(b, p, s == "-", pos)


def test_block_reverse_complement_vectors():
    for name in ("block_1", "block_2"):
        assert sr.block_reverse_complement(_block(MB[name])) == _block(MB[name + "_revcomp"])


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_merge_blocks_vectors(case):
    v = MB[case]
    g, edge, ids = sr.from_json(v["graph"]), _edge(v["edge"]), _new_ids(v["new_nodes"])
    pairings, new_nodes = sr.find_node_pairings(g, edge)
    assert pairings == {int(k): n for k, n in MB["pairings"].items()}
    assert {k: {f: n[f] for f in ("block_id", "path_id", "strand", "position")} for k, n in new_nodes.items()} == \
        {int(k): dict(n, position=tuple(n["position"])) for k, n in v["new_nodes"].items()}
    expected = _resolve(v["expected_graph"], ids)
    concat = sr.concatenate_alignments(_block(MB[v["concat_left"]]), _block(MB[v["concat_right"]]), pairings, ids)
    assert concat == expected["blocks"][1]                                      # list order inside every Edit included
    for update, field in ((sr.graph_merging_update_paths, "paths"), (sr.graph_merging_update_nodes, "nodes")):
        h = copy.deepcopy(g)
        update(h, new_nodes, 1)
        assert h[field] == expected[field]
    h = copy.deepcopy(g)
    sr.merge_blocks(h, edge)
    assert h == expected
    (only,) = sr.find_transitive_edges(g)
    assert sr.edge_eq(only, edge)
    assert sr.simplify(g, {p["name"] for p in g["paths"].values()}, [[only]]) == expected          # remove_transitive_edges
    # the product's graph level, the restatement standing in for the device
    assert sp.simplify(v["graph"], [None], merge=sr.merge_batch) == expected


def test_circularize_vectors():
    g = sr.from_json(CI["input_graph"])
    assert {b: len(blk["alignments"]) for b, blk in g["blocks"].items()} == {int(k): n for k, n in CI["block_depths"].items()}
    counts = sr.count_edges(g)
    for e, n in CI["edge_counts"]:
        assert [c for k, c in counts if sr.edge_eq(k, _edge(e))] == [n]
    for e in CI["absent_edges"]:
        assert not [c for k, c in counts if sr.edge_eq(k, _edge(e))]
    for graph, want in ((g, CI["transitive_edges"]), (sr.from_json(CI["single_block_graph"]), CI["single_block_transitive_edges"])):
        got = sr.find_transitive_edges(graph)
        assert len(got) == len(want) and all(sr.edge_eq(a, _edge(b)) for a, b in zip(got, want))
    assert [sr.conventional_orientation(e) for e in sr.find_transitive_edges(g)] == sp.find_transitive_edges(sp.normalize(CI["input_graph"]))
    # empty consensus sequences merge as well: the one transitive edge of the mock graph, through both implementations
    trace = {}
    got = sp.simplify(CI["input_graph"], [None], merge=sr.merge_batch, trace=trace)
    assert got == sr.simplify(g, {None}, trace["rounds"]) and len(got["blocks"]) == 3 and not sp.find_transitive_edges(got)


def test_simplify_run_vectors():
    g = sr.from_json(SR["graph"])
    h = copy.deepcopy(g)
    sr.remove_path(h, SR["remove_path"])
    assert h == sr.from_json(SR["after_remove_path"])
    h = sp.normalize(SR["graph"])
    sp.remove_path(h, SR["remove_path"])
    assert h == sr.from_json(SR["after_remove_path"])
    expected = sr.from_json(SR["expected_graph"])
    trace = {}
    got = sp.simplify(SR["graph"], SR["focal"], merge=sr.merge_batch, trace=trace)
    assert got == expected and set(got["nodes"]) >= {SR["NID11"], SR["NID12"]}
    assert sr.simplify(g, set(SR["focal"]), trace["rounds"]) == expected


# ---------------------------------------------------------------- the plasmid fixture
def _check_consistency(g):
    for nid, n in g["nodes"].items():
        assert n["block_id"] in g["blocks"] and n["path_id"] in g["paths"] and nid in g["blocks"][n["block_id"]]["alignments"]
    for bid, b in g["blocks"].items():
        assert len(b["alignments"]) == sum(1 for n in g["nodes"].values() if n["block_id"] == bid) and set(b["alignments"]) <= set(g["nodes"])
    assert sorted(n for p in g["paths"].values() for n in p["nodes"]) == sorted(g["nodes"])


@pytest.mark.parametrize("n_paths", PLASMID_COUNTS)
def test_plasmids_reduced_to_a_few_paths(plasmids, n_paths):
    G, names, genome = plasmids
    focal = names[:n_paths]
    before = sp.normalize(G)
    for pid in [pid for pid, p in before["paths"].items() if p["name"] not in focal]:
        sp.remove_path(before, pid)
    assert len(sp.find_transitive_edges(before)) > 0
    trace = {}
    g = sp.simplify(G, focal, merge=sr.merge_batch, trace=trace)
    for rnd in trace["rounds"]:
        used = [b for e in rnd for b in (e[0][0], e[1][0])]
        assert rnd and len(used) == len(set(used))
    assert not sp.find_transitive_edges(g) and not sr.find_transitive_edges(g)
    assert g == sr.simplify(sr.from_json(G), set(focal), trace["rounds"])
    _check_consistency(g)
    blocks, paths, kept = sg.recon_input(g)
    assert kept == focal
    for p, name in zip(paths, kept):
        assert rr.reconstruct_path(blocks, p) == genome[name]
    if n_paths == 1:
        assert len(trace["rounds"]) > 1


def test_all_paths_kept_leaves_the_graph_unchanged(plasmids):
    G, names, _ = plasmids
    calls = []
    g = sp.simplify(G, names, merge=lambda *a: calls.append(a))
    assert g == sr.from_json(G) and not calls and not sr.find_transitive_edges(g)


def test_a_schedule_is_checked():
    with pytest.raises(ValueError):
        sp.simplify(SR["graph"], SR["focal"], schedule=[[((1, "+"), (3, "+"))]], merge=sr.merge_batch)


# ---------------------------------------------------------------- the C interface
def test_merge_structs_match_the_header(tmp_path):
    import ctypes as C
    pairs = [("pga_merge_edge_t", sp.merge_edge_t), ("pga_merge_res_t", sp.merge_res_t), ("pga_merge_out_t", sp.merge_out_t)]
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


def test_library_exports_the_merge_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_merge_blocks", "pga_merge_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_merge_index_arithmetic_under_emulation_and_sanitizers(tmp_path):
    """pga_merge_idx.h: the tables and the three list kernels, then k_rows over the runs they built, against a direct scalar construction.
    k_merge_scan (wave intrinsics) is not part of the emulated program."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "merge_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "merge_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("merge_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------- what the GPU tests rely on their batches for
def test_generated_batches_hold_what_the_gpu_tests_rely_on():
    combos = {rc: 0 for rc in sg.RC}
    n_edges = status2 = boundary = unsorted = 0
    for seed in range(40):
        blocks, edges = sg.random_batch(seed)
        assert 2 <= len(blocks) <= 10 and 1 <= len(edges) <= 8
        status, b, u = sg.batch_facts(blocks, edges)
        for e in edges:
            combos[(e["left_rc"], e["right_rc"])] += 1
        n_edges += len(edges); status2 += sum(s == 2 for s in status); boundary += b; unsorted += u
    assert all(5 * n >= n_edges for n in combos.values()) and status2 >= 5 and boundary >= 5 and unsorted >= 5, (combos, n_edges, status2, boundary, unsorted)
    blocks, edges = sg.edge_batch()
    status, b, u = sg.batch_facts(blocks, edges)
    assert set(status) == {0} and b >= 4 and u >= 1
    assert {len(blk["consensus"]) for blk in blocks} >= set(sg.CONS_LENGTHS)
    named = [blocks[i] for e in edges for i in (e["left"], e["right"])]
    for kind in ("subs", "dels", "inss"):
        assert {len(m[kind]) for blk in named for m in blk["members"]} >= set(sg.LIST_LENGTHS)
    assert {len(s) for blk in named for m in blk["members"] for _, s in m["inss"]} >= set(sg.INS_LENGTHS)
    assert {(e["left_rc"], e["right_rc"]) for e in edges} == set(sg.RC) and {len(blk["members"]) for blk in named} >= {0, 1, 70}
    assert any(e["partner"] != sorted(e["partner"]) for e in edges)
    # a boundary merge under each of the four strand combinations
    for rc in sg.RC:
        assert any(sg.batch_facts(blocks, [e])[1] for e in edges if (e["left_rc"], e["right_rc"]) == rc)
