"""pga_remove_paths without a GPU: what the cases of tests/remove_gen.py hold (pinned on host_remove, which is simplify.remove_path path
by path and the expectation of the GPU tests), the ctypes mirrors against the header, simplify(paths=...) over a stand-in for the device
call (the packing and the reading back of pangraph_amd/remove.py), and the kernels of pga_remove_idx.h in a stand-alone program under the
host sanitizers (tests/emu/remove_emu.cpp)."""
import ctypes as C
import gzip
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import remove_gen as rg
import simplify_gen as sg
import simplify_ref as sr
import topo_gen as tg
from conftest import GOLDEN, ROOT
from pangraph_amd import remove as rm
from pangraph_amd import simplify as sp

VEC = json.load(open(os.path.join(GOLDEN, "simplify_vectors.json")))["simplify_run"]
PLASMID_COUNTS = (1, 3, 8)


def _kept(name):
    """per input member: whether it stays"""
    return [m >= 0 for m in rg.expected(name)["member_map"]]


# ---------------------------------------------------------------- every named case holds what it is named for
def test_reference_vector():
    c, exp = rg.case("reference"), rg.expected("reference")
    g = rm.graph_after(c["graph"], [b[0] for b in c["lists"][0]], (exp["blocks"], exp["paths"], exp["nodes"]), exp["dicts"])
    assert g == sr.from_json(VEC["after_remove_path"]) and c["keep"] == [False, True, True]
    h = sp.normalize(VEC["graph"])
    sp.remove_path(h, VEC["remove_path"])
    assert g == h                                                           # host_remove is path-by-path remove_path
    assert exp["counts"][:5] == (3, 2, 5, 5, 0) and exp["path_map"] == [-1, 0, 1]


def test_keep_all_and_keep_none():
    c, exp = rg.case("keep_all"), rg.expected("keep_all")
    members, subs, dels, inss, _ = rg.flat_of(c)
    assert (exp["blocks"], exp["paths"], exp["nodes"]) == c["lists"] and exp["dicts"] == c["dicts"] and exp["member_map"] == list(range(7))
    assert (exp["members"], exp["subs"], exp["dels"], exp["inss"]) == (members, subs, dels, inss) and subs and dels and inss
    exp = rg.expected("keep_none")
    assert exp["counts"] == (3, 0, 0, 0, 3, 0, 0, 0, 0) and exp["blocks"] == [(b[0], 0, 0, 0) for b in rg.case("keep_none")["lists"][0]]
    assert exp["member_map"] == [-1] * 7 and [len(d["consensus"]) for d in exp["dicts"]] == [b[1] for b in rg.case("keep_none")["lists"][0]]


def test_empty_paths_removed_and_kept():
    c, exp = rg.case("empty_path"), rg.expected("empty_path")
    assert [(p[2], k) for p, k in zip(c["lists"][1], c["keep"])] == [(0, False), (2, True), (0, True), (2, False)]
    assert exp["paths"] == [(2, 0, 2, 0), (3, 2, 0, 1)] and exp["path_map"] == [-1, 0, 1, -1]


def test_two_nodes_of_a_removed_path_in_one_block():
    c, exp = rg.case("one_block_twice"), rg.expected("one_block_twice")
    assert [n[3] for n in c["lists"][2]] == [0, 1, 0, 0, 2] and _kept("one_block_twice") == [False, False, True, False, True]
    assert exp["blocks"][0][2:] == (1, 1) and exp["nodes"][0][3:5] == (0, 0) and c["lists"][2][3][4] == 2        # slot 2 of A becomes slot 0


def test_a_block_dies_between_two_survivors():
    exp = rg.expected("dies")
    assert [b[3] for b in exp["blocks"]] == [1, 0, 1] and exp["blocks"][1] == (2, 0, 0, 0) and exp["rc_blocks"][1] == (rg.case("dies")["lists"][0][1][1], 0)
    assert exp["counts"][4] == 1 and [n[3] for n in exp["nodes"]] == [0, 2]


def test_a_block_dead_before():
    c, exp = rg.case("dead_before"), rg.expected("dead_before")
    assert c["lists"][0][1] == (77, 7, 3, 0) and exp["blocks"][1] == (77, 0, 0, 0) and [b[3] for b in exp["blocks"]] == [1, 0, 1, 1]
    assert {n[3] for n in c["lists"][2]} == {0, 2, 3} and exp["rc_blocks"][1][1] == 0


def test_removed_circular_path_wraps_in_kept_blocks():
    c, exp = rg.case("wrap_node"), rg.expected("wrap_node")
    first, last = c["lists"][2][0], c["lists"][2][2]
    assert c["lists"][1][0][3] == 1 and not c["keep"][0] and exp["blocks"][first[3]][3] == 1 and exp["blocks"][last[3]][3] == 1 and exp["blocks"][1][3] == 0
    assert exp["paths"] == [(2, 0, 2, 0)]


@pytest.mark.parametrize("n", [rg.TILE - 1, rg.TILE, rg.TILE + 1])
def test_tile_edges(n):
    c, exp = rg.case(f"tile_{n}"), rg.expected(f"tile_{n}")
    kept = _kept(f"tile_{n}")
    assert len(kept) == len(c["lists"][2]) == n and kept[-2:] == [True, False] and kept[0] and not kept[(n - 2) // 3] and kept[n - 3]
    assert 0 < exp["counts"][5] and 0 < exp["counts"][7] and exp["nodes"][-1][4] < c["lists"][2][-1][4]


def test_second_level_of_the_tile_scan():
    inp, exp = rg.second_level()
    n = rg.TILE * rg.SCAN_THREADS
    assert len(inp["members"]) > n and 0 < exp["kept"][:n].sum() < n and 0 < exp["kept"][n:].sum() < len(exp["kept"]) - n
    assert exp["member_map"][n + 3] == -1 and exp["member_map"][-1] == exp["kept"].sum() - 1 and len(exp["subs"]) > rg.TILE and len(exp["inss"]) > rg.TILE
    # the numpy expectation is host_remove's on a small graph of the same make
    small, (_, x) = rg.second_level_case(64), rg.second_level(64)
    for flags in (0, rm.COMPACT_LETTERS):
        e = rg.host_remove(small, flags)
        rows = lambda a: [tuple(int(v) for v in r) for r in a.tolist()]
        assert [r[:3] + r[3:6] for r in rows(x["nodes"])] == [n_[:6] for n_ in e["nodes"]] and rows(x["paths"]) == e["paths"]
        assert [r[:4] for r in rows(x["blocks"])] == e["blocks"] and rows(x["members"]) == e["members"] and rows(x["subs"]) == e["subs"] and rows(x["dels"]) == e["dels"]
        assert rows(x["inss_compact"] if flags else x["inss"]) == e["inss"] and x["member_map"].tolist() == e["member_map"] and x["path_map"].tolist() == e["path_map"]
        assert not flags or bytes(x["ins_seq"]) == e["ins_seq"]


def test_skew():
    c, exp = rg.case("skew"), rg.expected("skew")
    members = rg.flat_of(c)[0]
    assert [m[0] for m in members].count(5000) == 2 and [m[2] for m in members].count(3000) == 2 and sum(1 for m in members if m == (0, 0, 0)) == 2000
    kept = _kept("skew")
    assert kept == [True] * 1001 + [False] * 1001 and members[0][0] == members[1001][0] == 5000 and exp["counts"][5:8] == (5000, 7, 3000)


def test_offsets():
    c, exp = rg.case("offsets"), rg.expected("offsets")
    members = rg.flat_of(c)[0]
    assert _kept("offsets") == [False, True] * 6 and members[0::2] == [(3, 5, 7)] * 6 and members[1::2] == [(n, n, n) for n in sg.LIST_LENGTHS]
    assert exp["members"] == [(n, n, n) for n in sg.LIST_LENGTHS]


def test_letters():
    c = rg.case("letters")
    seq, offs = c["letters"]
    _, _, _, inss, _ = rg.flat_of(c)
    assert [ln for _, ln, _ in inss] == list(sg.INS_LENGTHS) * 3 and offs != sorted(offs) and offs[11] == offs[1] and len(set(offs)) == 14
    plain, compact = rg.expected("letters"), rg.expected("letters", rm.COMPACT_LETTERS)
    assert plain["ins_seq"] is None and [x[2] for x in plain["inss"]] == offs[:5] + offs[10:]
    assert [x[2] for x in compact["inss"]] == [sum(x[1] for x in compact["inss"][:k]) for k in range(10)] and len(compact["ins_seq"]) == 2 * sum(sg.INS_LENGTHS)
    assert plain["dicts"] == compact["dicts"] and compact["ins_seq"] == "".join(s for m in compact["dicts"][0]["members"] for _, s in m["inss"]).encode()


def test_block_index_above_2_16():
    c, exp = rg.case("high_block_index"), rg.expected("high_block_index")
    assert min(n[3] for n in c["lists"][2]) > 1 << 16 and exp["counts"][4] == (1 << 16) + 5 + 1
    assert exp["blocks"][-3:] == rg.expected("one_block_twice")["blocks"] and [n[3] - (1 << 16) - 5 for n in exp["nodes"]] == [n[3] for n in rg.expected("one_block_twice")["nodes"]]


def test_random_graphs_hold_what_the_gpu_tests_rely_on():
    n_removed = n_died = n_dead_in = n_kept_paths = n_renumbered = n_circ = n_letters = 0
    for seed in range(40):
        c = rg.random_case(seed)
        exp = rg.host_remove(c)
        n_removed += exp["member_map"].count(-1)
        n_died += sum(1 for a, b in zip(c["lists"][0], exp["blocks"]) if a[3] and not b[3])
        n_dead_in += sum(1 for b in c["lists"][0] if not b[3])
        n_kept_paths += len(exp["paths"])
        n_circ += sum(1 for p, k in zip(c["lists"][1], c["keep"]) if p[3] and p[2] and not k)
        n_letters += bool(c["letters"])
        by_id = {n[0]: n for n in c["lists"][2]}
        n_renumbered += sum(1 for n in exp["nodes"] if by_id[n[0]][4] != n[4])
    assert n_removed >= 100 and n_died >= 20 and n_dead_in >= 10 and n_kept_paths >= 30 and n_renumbered >= 20 and n_circ >= 10 and n_letters == 10, \
        (n_removed, n_died, n_dead_in, n_kept_paths, n_renumbered, n_circ, n_letters)


def test_expected_edits_are_the_surviving_alignments():
    """the flat layout (the input's arrays filtered) decodes to the alignments remove_path left"""
    for c, flags in [(rg.case(n), f) for n in ("reference", "letters", "offsets", "dead_before") for f in (0, 1)] + [(rg.random_case(s), s & 1) for s in range(12)]:
        exp = rg.host_remove(c, flags)
        seq = exp["ins_seq"] if flags else rg.flat_of(c)[4]
        s = d = i = 0
        members = iter(exp["members"])
        for blk in exp["dicts"]:
            for e in blk["members"]:
                ns, nd, ni = next(members)
                assert e["subs"] == [(p, chr(a)) for p, a in exp["subs"][s:s + ns]] and e["dels"] == exp["dels"][d:d + nd]
                assert e["inss"] == [(p, seq[off:off + ln].decode()) for p, ln, off in exp["inss"][i:i + ni]]
                s += ns; d += nd; i += ni
        g = rg.graph_after(c)
        bids = [b[0] for b in c["lists"][0]]
        assert rm.graph_after(rg.to_graph(c["lists"], c["dicts"])[0], bids, (exp["blocks"], exp["paths"], exp["nodes"]), exp["dicts"]) == g


# ---------------------------------------------------------------- the C interface
def test_remove_structs_match_the_header(tmp_path):
    pairs = [("pga_remove_out_t", rm.remove_out_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  printf("%u\\n", PGA_REMOVE_COMPACT_LETTERS);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp + [[str(rm.COMPACT_LETTERS)]]


def test_library_exports_the_remove_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_remove_paths", "pga_remove_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_numpy_mirrors_have_the_sizes_of_the_structs():
    from pangraph_amd.reconsensus import rc_block_t
    assert rg.NP_RC.itemsize == C.sizeof(rc_block_t) and rg.NP_NODE.itemsize == 40 and rg.NP_INS.itemsize == 16 and rg.NP_SUB.itemsize == rg.NP_DEL.itemsize == 8


# ---------------------------------------------------------------- simplify(paths=stand-in): packing and reading back without a device
def stand_in(calls=None):
    def call(blocks, paths, nodes, dicts, keep):
        exp = rg.host_remove({"lists": (blocks, paths, nodes), "dicts": dicts, "keep": keep, "letters": None})
        if calls is not None:
            calls.append(keep)
        return {"blocks": exp["blocks"], "paths": exp["paths"], "nodes": exp["nodes"], "dicts": exp["dicts"]}
    return call


def _both(graph, focal, **kw):
    calls, t0, t1 = [], {}, {}
    want = sp.simplify(graph, focal, merge=sr.merge_batch, trace=t0, **kw)
    got = sp.simplify(graph, focal, merge=sr.merge_batch, trace=t1, paths=stand_in(calls), **kw)
    assert got == want and t0["rounds"] == t1["rounds"] and len(calls) == 1
    return got, calls[0]


def test_stand_in_on_the_reference_vector():
    got, keep = _both(VEC["graph"], VEC["focal"])
    assert got == sr.from_json(VEC["expected_graph"]) and keep == [True, True, False]
    _both(VEC["graph"], VEC["focal"], topology=tg.host_plan)
    _both(VEC["graph"], ["pathB", "pathC"])


@pytest.fixture(scope="module")
def plasmids():
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    return G, [G["paths"][k]["name"] for k in sorted(G["paths"], key=int)]


@pytest.mark.parametrize("n_paths", PLASMID_COUNTS)
def test_stand_in_on_the_plasmids(plasmids, n_paths):
    G, names = plasmids
    got, keep = _both(G, names[:n_paths])
    assert sum(keep) == n_paths and len(keep) == len(names) and not sp.find_transitive_edges(got)
    if n_paths == 3:
        _both(G, names[:n_paths], topology=tg.host_plan)


def test_stand_in_on_random_graphs():
    n_rounds = 0
    for seed in range(12):
        c = rg.random_case(seed)
        g, _, _ = rg.to_graph(c["lists"], c["dicts"])
        focal = [f"p{p[0]}" for p, k in zip(c["lists"][1], c["keep"]) if k]
        want = sp.simplify(g, focal, merge=sr.merge_batch)
        trace = {}
        assert sp.simplify(g, focal, merge=sr.merge_batch, paths=stand_in(), trace=trace) == want
        assert sp.simplify(g, focal, merge=sr.merge_batch, paths=stand_in(), topology=tg.host_plan) == want
        n_rounds += len(trace["rounds"])
    assert n_rounds >= 5


def test_default_arguments_do_not_touch_the_new_module(monkeypatch):
    monkeypatch.setattr(rm, "removed_graph", lambda *a, **k: (_ for _ in ()).throw(AssertionError("simplify() with default arguments called pga_remove_paths")))
    assert sp.simplify(VEC["graph"], VEC["focal"], merge=sr.merge_batch) == sr.from_json(VEC["expected_graph"])


# ---------------------------------------------------------------- the kernels on the host
def test_remove_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_remove_idx.h: validation, the graph checks of pga_topo_idx.h, every kernel (the tile scans with several quantities, the list copies
    over more than one tile, the letters) against a direct scalar construction, and every refusal"""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "remove_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "remove_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("remove_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)
