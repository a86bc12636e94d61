"""pga_join_graphs without a device: the cases of tests/join_gen.py pinned on what graph_join says about them, host_join (the dict route)
against flat_join (the header's text in loops over the tables), the ctypes mirrors against the header, the leaves, the graph level with a
stand-in for the call, and the kernels of pga_join_idx.h under the emulation and the host sanitizers (tests/emu/join_emu.cpp)."""
import copy
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import join_gen as jg
from conftest import GOLDEN, ROOT
from pangraph_amd import close as cl
from pangraph_amd import join as jn


def _ids(k, f):
    return [[x[0] for x in p["t"][f] if f != "blocks" or x[3]] for p in k["parts"]]


# ---------------------------------------------------------------- the cases hold what their names say
def test_every_case_is_the_sorted_union_of_its_parts():
    for name, k in jg.all_cases():
        e = k["exp"]
        for f in ("blocks", "paths"):
            want = sorted(x for ids in _ids(k, f) for x in ids)
            assert [x[0] for x in e[f]] == want and len(set(want)) == len(want), (name, f)
        assert sorted(n[0] for n in e["nodes"]) == sorted(x for ids in _ids(k, "nodes") for x in ids), name
        assert e["totals"][3] == sum(len(p["t"]["who"]) for p in k["parts"]) and e["totals"][8] == int(e["inss"]["len"].sum()), name
        off, run = e["inss"]["seq_off"].astype(np.int64), np.concatenate([[0], np.cumsum(e["inss"]["len"].astype(np.int64))])[:-1]
        assert (off == run).all(), name
        at = 0
        for p in e["paths"]:                                                     # node_off is the running sum
            assert p[1] == at, name
            at += p[2]
        for m, (n, rev) in enumerate(e["who"]):                                  # a member after is the member of its part that carries the same node
            assert tuple(k["parts"][e["origin_part"][m]]["t"]["who"][e["origin"][m]]) == (n, rev), name


def test_leaf_merge_and_id_orders():
    e = jg.case("two_singletons")["exp"]
    assert [b[0] for b in e["blocks"]] == [3, 5] and e["block_map"] == [1, 0] and e["path_map"] == [1, 0] and e["origin_part"] == [1, 0] and e["origin"] == [0, 0]
    assert e["nodes"] == [(3, 0, 25, 0, 0, 1), (5, 0, 0, 1, 0, 0)] and e["paths"] == [(3, 0, 1, 0), (5, 1, 1, 1)]
    e = jg.case("alternating")["exp"]
    assert [b[0] % 2 for b in e["blocks"]] == [0, 1] * 11 and e["block_map"][:11] == list(range(0, 22, 2))
    assert jg.case("left_below")["exp"]["block_map"] == list(range(12))
    assert jg.case("left_above")["exp"]["block_map"] == list(range(7, 12)) + list(range(7))
    e = jg.case("id_extremes")["exp"]
    assert [b[0] for b in e["blocks"]] == [0, 1, 1 << 63, (1 << 64) - 1]


def test_dead_entries_and_empty_parts():
    k = jg.case("one_part_dead_entries")
    t, e = k["parts"][0]["t"], k["exp"]
    assert [b[3] for b in t["blocks"]][:3] == [0, 0, 1] and [b[3] for b in t["blocks"]].count(0) == 5 and e["block_map"].count(jg.NONE) == 5
    assert e["origin"] == list(range(len(t["who"]))) and set(e["origin_part"]) == {0} and e["totals"][0] == len(t["blocks"]) - 5
    k = jg.case("empty_parts")
    assert [len(p["t"]["blocks"]) for p in k["parts"]] == [0, 5, 0, 2, 0] and k["exp"]["block_map_off"] == [0, 0, 5, 5, 7, 7] and set(k["exp"]["origin_part"]) == {1, 3}


def test_part_counts():
    assert len(jg.case("three_parts")["parts"]) == 3 and len(jg.case("eight_parts")["parts"]) == 8
    k = jg.case("singletons_1025")
    assert len(k["parts"]) == 1025 and k["exp"]["totals"][:5] == (1025, 1025, 1025, 1025, 1025) and k["exp"]["block_map"] != sorted(k["exp"]["block_map"])


def test_strands_paths_and_slots():
    k = jg.case("reverse_circular_empty_path")
    e = k["exp"]
    assert any(n[5] for n in e["nodes"]) and any(p[3] for p in e["paths"]) and [p[2] for p in e["paths"]].count(0) >= 2 and e["paths"][0][2] == 0 and e["paths"][-1][2] == 0
    e = jg.case("two_nodes_of_one_path")["exp"]
    assert len(e["paths"]) == 2 and sorted(p[2] for p in e["paths"]) == [4, 5]
    assert any(n[3] > 1 << 16 for n in jg.case("high_index")["exp"]["nodes"])


def test_sizes_at_the_tile_edges():
    for n in (cl.TILE - 1, cl.TILE, cl.TILE + 1):
        assert n in [b[2] for b in jg.case(f"members_{n}")["exp"]["blocks"]]
        assert n in [p[2] for p in jg.case(f"path_{n}")["exp"]["paths"]]
    e = jg.case("straddle")["exp"]
    first = np.concatenate([[0], np.cumsum([b[2] for b in e["blocks"]])])
    assert any(first[i] < cl.TILE < first[i + 1] and b[2] == 100 for i, b in enumerate(e["blocks"]))
    c = jg.case("one_heavy")["exp"]["counts"]
    assert (c[:, 0] == 5000).sum() == 1 and (c[:, 2] == 3000).sum() == 1 and (c.sum(axis=1) == 0).sum() >= 2000
    c = jg.case("list_lengths")["exp"]["counts"]
    assert set(range(131)) <= set(c[:, 0].tolist()) and c.max() == 130
    assert jg.case("second_level")["exp"]["totals"][5] > cl.TILE * cl.TILE


def test_letters_shared_shuffled_and_dense():
    k = jg.case("letters")
    assert {0, 1, 63, 64, 65, 127, 128, 5000} <= set(k["exp"]["inss"]["len"].tolist())
    off = k["parts"][0]["t"]["inss"]["seq_off"].astype(np.int64)
    assert len(set(off.tolist())) < len(off) and (np.diff(off) < 0).any()           # shared and shuffled in one part
    i1 = k["parts"][1]["t"]["inss"]
    assert (i1["seq_off"].astype(np.int64) == np.concatenate([[0], np.cumsum(i1["len"].astype(np.int64))])[:-1]).all()   # dense in the other
    k = jg.case("buffer_end")
    assert len(k["parts"][0]["t"]["ins_seq"]) > len(k["parts"][1]["t"]["ins_seq"])


def test_random_joins_hold_what_the_gpu_tests_rely_on():
    sizes, dead = set(), 0
    for s in range(40):
        k = jg.random_case(s)
        sizes.add(len(k["parts"]))
        dead += k["exp"]["block_map"].count(jg.NONE)
    assert sizes == {2, 3, 4, 5} and dead >= 10


# ---------------------------------------------------------------- the two restatements, the conflicts
def test_restated_call_agrees_with_host_join():
    for name, k in jg.all_cases():
        if name != "second_level":                                               # (a million records in a Python loop)
            assert jg.same(jg.flat_join([p["t"] for p in k["parts"]]), k["exp"]) is None, name


def conflict_parts(kind):
    """two parts of the `alternating` case that share one id of the kind (or, for "node_within", a part that holds a node id twice) -> (tables, the id)"""
    tables = [copy.deepcopy(p["t"]) for p in jg.case("alternating")["parts"]]
    a, b = tables
    if kind == "block":
        i, j = [i for i, x in enumerate(a["blocks"]) if x[3]][-1], [i for i, x in enumerate(b["blocks"]) if x[3]][-1]
        ident = max(a["blocks"][i][0], b["blocks"][j][0]) + 10
        a["blocks"][i], b["blocks"][j] = (ident,) + tuple(a["blocks"][i][1:]), (ident,) + tuple(b["blocks"][j][1:])
    elif kind == "path":
        ident = max(a["paths"][-1][0], b["paths"][-1][0]) + 10
        a["paths"][-1], b["paths"][-1] = (ident,) + tuple(a["paths"][-1][1:]), (ident,) + tuple(b["paths"][-1][1:])
    elif kind == "node":
        ident = a["nodes"][3][0]
        b["nodes"][2] = (ident,) + tuple(b["nodes"][2][1:])
    else:
        ident = b["nodes"][5][0]
        b["nodes"][1] = (ident,) + tuple(b["nodes"][1][1:])
    return tables, ident


@pytest.mark.parametrize("kind", ["block", "path", "node", "node_within"])
def test_conflicts_are_refused_by_both_restatements(kind):
    tables, ident = conflict_parts(kind)
    with pytest.raises(jn.JoinError, match=f"Conflicting key: {kind.split('_')[0]} id {ident} "):
        jg.flat_join(tables)
    if kind != "node_within":                                                    # (a dict cannot hold a key twice)
        parts = jg.case("alternating")["parts"]
        f = kind + "s"
        left, right = copy.deepcopy(parts[0]["g"]), copy.deepcopy(parts[1]["g"])
        key = sorted(left[f])[0]
        right[f][key] = left[f][key]
        with pytest.raises(jn.JoinError, match=f"Conflicting key: '{key}'"):
            jn.graph_join(left, right)


def test_graph_join_is_the_union():
    parts = jg.case("three_parts")["parts"]
    g = jn.graph_join(jn.graph_join(parts[0]["g"], parts[1]["g"]), parts[2]["g"])
    for f in ("blocks", "paths", "nodes"):
        assert len(g[f]) == sum(len(p["g"][f]) for p in parts) and all(g[f][x] is p["g"][f][x] for p in parts for x in p["g"][f])


# ---------------------------------------------------------------- the leaves
def test_singleton_tables_are_the_dict_singleton():
    for index, seq, circular, reverse in [(7, "ACGTTGCA", False, False), (0, "A", True, True), ((1 << 64) - 1, "ACGT" * 50, True, False), (12, "", False, True)]:
        g = jn.singleton_graph(index, seq, circular, reverse)
        want, _ = cl.graph_tables(g)
        got = jn.singleton_tables(index, seq, circular, reverse)
        assert list(g["blocks"]) == list(g["paths"]) == list(g["nodes"]) == [index] and g["nodes"][index]["position"] == ((0, 0) if circular else (0, len(seq)))
        for f in ("blocks", "paths", "nodes", "rc_blocks", "subs", "dels", "inss", "who"):
            assert [tuple(x) for x in got[f]] == [tuple(x) for x in want[f]], f
        assert [tuple(c) for c in got["counts"]] == [tuple(c) for c in want["counts"]] == [(0, 0, 0)] and got["ins_seq"] == want["ins_seq"] == b""
        jn.Tables(got)


# ---------------------------------------------------------------- the C interface
def test_join_structs_match_the_header(tmp_path):
    pairs = [("pga_join_part_t", jn.join_part_t), ("pga_join_out_t", jn.join_out_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  printf("%u\\n", PGA_JOIN_COPY_CONSENSUS);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp + [[str(jn.COPY_CONSENSUS)]]


def test_library_exports_the_join_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_join_graphs", "pga_join_free", "pga_join_last_ms"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_tables_pack_what_the_part_holds():
    t = jg.case("letters")["parts"][0]["t"]
    K = jn.Tables(t)
    g, b, who, n = jn._part(K)
    assert g[0] == b[0] == len(t["blocks"]) and n == len(t["ins_seq"]) and [(w["node_id"], w["reverse"]) for w in who] == t["who"]
    g2, b2, who2, n2 = jn._part((K, K.W, 7))
    assert n2 == 7 and who2 is K.W and g2 is g


# ---------------------------------------------------------------- the kernels on the host
def test_join_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_join_idx.h on every named case of tests/join_gen.py (dumped to a file each, held against host_join's expectation and a scalar
    construction) and on random instances: validation, every kernel (the keys, the insertion ranges, the ranks, the scans, the descriptors, the nodes, the slot
    check, the list copies and the letter gather of pga_assemble_idx.h), every refusal of the host and of the kernels."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "join_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "join_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    files = []
    for name in jg.CASES:
        files.append(str(tmp_path / f"{name}.bin"))
        jg.dump(jg.case(name), files[-1])
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith(f"join_emu OK ({len(jg.CASES)} named cases") and not noise, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------- merge_pair(join=stand-in): the tables and the reading back without a device
def split(g):
    """a graph cut in two along its paths: the paths that share a block (directly or through others) with the first one and their blocks, and the rest"""
    left_p, left_b = set(), set()
    todo = [min(g["paths"])] if g["paths"] else []
    blocks_of = {p: {g["nodes"][n]["block_id"] for n in v["nodes"]} for p, v in g["paths"].items()}
    while todo:
        p = todo.pop()
        if p in left_p:
            continue
        left_p.add(p)
        left_b |= blocks_of[p]
        todo += [q for q in g["paths"] if q not in left_p and blocks_of[q] & left_b]
    take = lambda keep_p, keep_b: {"paths": {p: v for p, v in g["paths"].items() if keep_p(p)}, "blocks": {b: v for b, v in g["blocks"].items() if keep_b(b)},
                                   "nodes": {n: v for n, v in g["nodes"].items() if keep_p(v["path_id"])}}
    return take(lambda p: p in left_p, lambda b: b in left_b), take(lambda p: p not in left_p, lambda b: b not in left_b)


def test_stand_in_join_against_the_join_in_dicts(oracle_lib):
    import apply_gen as ag
    import detach_ref as dr
    import promise_ref as pr
    import reweave_gen as rg
    import reweave_ref as rr
    from test_close_cpu import _round, fake_reconsensus
    vec = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
    solve = lambda promises: [pr.solve_promise(oracle_lib.dll, q) for q in promises]
    kw = dict(solve=solve, plan=rr.expected_call, slicer=ag.ref_slicer, detach=dr.expected_call, rc=fake_reconsensus)
    calls = []

    def stand_in(tables, flags):
        calls.append([len(t["blocks"]) for t in tables])
        for t in tables:
            jn.Tables(t)                                                         # (the tables pack)
        return jg.flat_join(tables, flags)

    def both(make, thr):
        (l0, r0, matches), (l1, r1, _) = make(), make()
        want = _round(lambda: jn.merge_pair(l0, r0, [matches], thr, **kw))
        got = _round(lambda: jn.merge_pair(l1, r1, [matches], thr, join=stand_in, **kw))
        assert got == want
        return want

    def from_vector():
        g, matches = rg.reference_graph(vec)
        left, right = split(g)
        assert jn.graph_join(left, right).keys() == g.keys() and all(jn.graph_join(left, right)[f] == g[f] for f in g)
        return left, right, matches

    def from_random(seed):
        left, matches = ag.random_graph(seed)
        right = jg.relabel(jg.graph(seed, {50: (20, 3), 60: (30, 2)}), path=lambda p: 3 * p)
        return left, right, matches

    assert both(from_vector, vec["reweave"]["thr_len"]) != "MergeError"
    done = [both(lambda: from_random(seed), rg.THR) != "MergeError" for seed in range(40)]
    assert sum(done) >= 6 and len(calls) == 41 and all(len(c) == 2 for c in calls) and sum(1 for c in calls if min(c) > 0) >= 40
    assert _round(lambda: jn.merge_pair(*from_random(0)[:2], [], rg.THR, join=stand_in)) == _round(lambda: jn.graph_join(*from_random(0)[:2]))   # (no round: the join alone)
