"""pga_close_round without a device: the cases of tests/close_gen.py pinned on what tests/detach_ref.py says about them, host_close (the dict
route) against flat_close (the header's text in loops over the tables), the ctypes mirrors against the header, the list level's packing, the
graph level with stand-ins for every device call, and the kernels of pga_close_idx.h (with pga_rc_detach_args) under the emulation and the
host sanitizers (tests/emu/close_emu.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import close_gen as cg
import detach_ref as dr
from conftest import ROOT
from pangraph_amd import close as cl
from pangraph_amd import detach as dt


def _orphans(k):
    return len(k["d1"]["orphans"]), len(k["d2"]["orphans"])


# ---------------------------------------------------------------- the cases hold what their names say
def test_no_orphan_has_every_kind():
    k = cg.case("no_orphan")
    assert _orphans(k) == (0, 0) and sorted(k["exp"]["kinds"]) == [0, 1, 2] and k["exp"]["totals"][0] == len(k["t"]["blocks"])
    assert k["exp"]["block_map"] == list(range(5)) and k["exp"]["origin"] == list(range(14))
    upd = k["t"]["upd"]
    for j, b in enumerate(upd):                                                  # kind 0 keeps its letters, 1 and 2 get the reconsensus'
        kind, cons = k["t"]["rc"]["blocks"][j]
        assert k["exp"]["rc_blocks"][b][0] == (cons if kind else k["t"]["rc_blocks"][b][0]) and (kind == 0) == (cons == k["t"]["rc_blocks"][b][0])


def test_orphans_of_either_stage():
    assert _orphans(cg.case("first_only")) == (2, 0) and _orphans(cg.case("second_only")) == (0, 4) and _orphans(cg.case("both_in_one_block")) == (2, 2)
    k = cg.case("both_in_one_block")
    e = k["exp"]
    j = [i for i, b in enumerate(e["blocks"]) if b[0] == 70][0]
    assert e["blocks"][j][2] == 1 and sorted(o[3] for o in e["orphans"]) == [i for i, b in enumerate(e["blocks"]) if b[0] in {o[2] for o in e["orphans"]}]
    for member, nid, bid, block, ln, status in e["orphans"]:                     # the node of an orphan: same id, the singleton, slot 0, forward
        node = [n for n in e["nodes"] if n[0] == nid][0]
        assert (node[3], node[4], node[5]) == (block, 0, 0) and e["blocks"][block] == (bid, ln, 1, 1) and e["who"][sum(b[2] for b in e["blocks"][:block])] == (nid, 0)
        assert k["t"]["who"][member][0] == nid and bid == dr.block_id(nid, e["rc_blocks"][block][0].decode())


def test_block_that_loses_every_member_stays():
    e = cg.case("block_loses_every_member")["exp"]
    assert [b for b in e["blocks"] if b[0] in (50, 80)] == [(50, e["blocks"][[b[0] for b in e["blocks"]].index(50)][1], 0, 1), (80, e["blocks"][[b[0] for b in e["blocks"]].index(80)][1], 0, 1)]
    assert e["totals"][4] == 5


def test_reverse_and_empty_orphans():
    k = cg.case("reverse_orphan")
    (member, nid, bid, block, ln, _), = k["exp"]["orphans"]
    assert k["t"]["who"][member] == (nid, 1) and k["exp"]["who"][sum(b[2] for b in k["exp"]["blocks"][:block])] == (nid, 0)
    assert k["exp"]["rc_blocks"][block][0] == b"TGCAACGT"                        # the reverse complement of what the member inserted
    e = cg.case("empty_orphan")["exp"]
    assert [o[4] for o in e["orphans"]] == [0] * 4 and all(e["rc_blocks"][o[3]] == (b"", 1) for o in e["orphans"])


def test_singleton_ids_around_the_survivors():
    e = cg.case("id_ranges")["exp"]
    ids = [b[0] for b in e["blocks"]]
    sing = {o[2] for o in e["orphans"]}
    kinds = "".join("o" if b in sing else "s" for b in ids)
    assert ids == sorted(ids) and kinds.startswith("so") and "oso" in kinds and ids[-1] == (1 << 64) - 1 and kinds[:2] == "so" and kinds.count("o") == 4
    assert min(sing) < sorted(set(ids) - sing)[1] and kinds.rstrip("s").endswith("o")


def test_singletons_in_front_of_every_survivor():
    """both orphans' ids lie below the id of the updated block they left: the blocks after begin with the singletons"""
    e = cg.case("singleton_first")["exp"]
    sing = {o[2] for o in e["orphans"]}
    assert len(sing) == 2 and [b[0] in sing for b in e["blocks"]] == [True, True, False, False] and e["block_map"] == [2, 3] and sorted(o[3] for o in e["orphans"]) == [0, 1]


def test_two_nodes_of_one_path_and_dead_entries():
    k = cg.case("two_nodes_of_one_path")
    assert len(k["exp"]["paths"]) == 1 and k["exp"]["totals"][4] == 2 and [n[:3] for n in k["exp"]["nodes"]] == [n[:3] for n in k["t"]["nodes"]]
    k = cg.case("dead_entries")
    assert [b[3] for b in k["t"]["blocks"]].count(0) == 4 and k["exp"]["block_map"].count(cl.NONE) == 4 and len(k["exp"]["blocks"]) == len(k["t"]["blocks"]) - 4 + 1


def test_sizes_at_the_tile_edge_and_above_2_16():
    assert any(n[3] > 1 << 16 for n in cg.case("high_index")["exp"]["nodes"])
    for n in (cl.TILE - 1, cl.TILE, cl.TILE + 1):
        t = cg.case(f"members_{n}")["t"]
        assert t["blocks"][t["upd"][0]][2] == n
    t = cg.case("straddle")["t"]
    assert t["blocks"][0][2] == 1000 and t["blocks"][t["upd"][0]][2] == 100
    for name in ("one_heavy", "one_heavy_updated"):
        c = cg.case(name)["exp"]["counts"]
        assert (c[:, 0] == 5000).sum() == 1 and (c[:, 2] == 3000).sum() == 1 and (c.sum(axis=1) == 0).sum() >= 2000
    c = cg.case("list_lengths")["exp"]["counts"]
    assert set(range(131)) <= set(c[:, 0].tolist()) and c.max() == 130
    k = cg.case("letters")
    assert {0, 1, 63, 64, 65, 127, 128, 5000} <= set(k["exp"]["inss"]["len"].tolist())
    for inss in (k["t"]["inss"], k["t"]["redetached"]["inss"]):                   # shared, shuffled and overlapping offsets in both sources
        off = inss["seq_off"].astype(np.int64)
        assert len(set(off.tolist())) < len(off) and (np.diff(off) < 0).any()
    assert cg.case("second_level")["exp"]["totals"][5] > cl.TILE * cl.TILE
    assert cg.case("no_update")["t"]["upd"] == [] and cg.case("no_update")["exp"]["totals"][4] == 0


def test_random_rounds_hold_what_the_gpu_tests_rely_on():
    n1 = n2 = emptied = 0
    for s in range(40):
        k = cg.random_case(s)
        a, b = _orphans(k)
        n1, n2 = n1 + a, n2 + b
        emptied += sum(1 for j, i in enumerate(k["t"]["upd"]) if k["t"]["blocks"][i][2] and not k["t"]["redetached"]["n_members"][j])
    assert n1 >= 40 and n2 >= 20 and emptied >= 3, (n1, n2, emptied)


# ---------------------------------------------------------------- the two restatements
def test_restated_call_agrees_with_host_close():
    for name, k in cg.all_cases():
        if name != "second_level":                                               # (a million records in a Python loop)
            assert cg.same(cg.flat_close(k["t"]), k["exp"]) is None, name


def test_second_detach_on_every_block_equals_the_reference_route():
    """host_close detaches the kind-2 blocks only, as reconsensus_graph does; the tables hold a second detach over all updated blocks"""
    for name, k in cg.all_cases():
        for j, b in enumerate(k["spec"]["upd"]):
            if k["spec"]["rc"][b][0] != 2:
                assert k["t"]["redetached"]["n_members"][j] == k["t"]["detached"]["n_members"][j], name


# ---------------------------------------------------------------- the C interface
def test_close_structs_match_the_header(tmp_path):
    pairs = [("pga_close_out_t", cl.close_out_t), ("pga_detach_out_t", dt.detach_out_t), ("pga_detach_orphan_t", dt.detach_orphan_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  printf("%u %d\\n", PGA_CLOSE_COPY_CONSENSUS, PGA_ASSEMBLE_TILE);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp + [[str(cl.COPY_CONSENSUS), str(cl.TILE)]]
    for name, _ in dt.detach_orphan_t._fields_:
        assert cl.ORPHAN.fields[name][1] == getattr(dt.detach_orphan_t, name).offset, name


def test_library_exports_the_close_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_close_round", "pga_close_free", "pga_close_last_ms", "pga_rc_detach_args"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_tables_pack_what_the_case_holds():
    k = cg.case("both_in_one_block")
    t = k["t"]
    K = cl.Tables(t)
    graph, block_args, n_letters, who, upd, d1, rc, rc_len, d2 = K.call_args()
    assert graph[0] == len(t["blocks"]) == block_args[0] and n_letters == len(t["ins_seq"]) and upd == t["upd"] and rc_len == len(t["rc"]["ins_seq"])
    assert [(who[m]["node_id"], who[m]["reverse"]) for m in range(len(t["who"]))] == t["who"]
    assert (d1.n_blocks, d1.n_orphans, d2.n_blocks, d2.n_orphans) == (3, 2, 3, 2)
    assert [d1.member_map[m] for m in range(5)] == t["detached"]["member_map"] and [d2.member_map[m] for m in range(3)] == t["redetached"]["member_map"]
    for d, rows in ((d1, t["detached"]["orphans"]), (d2, t["redetached"]["orphans"])):
        for i, o in enumerate(rows):
            r = d.orphans[i]
            at = C.c_void_p.from_address(C.addressof(d.blocks[r.block])).value
            assert (r.member, r.node_id, r.block_id, r.len, r.status, r.block) == o[:5] + (1 + i,) and C.string_at(at, r.len) == o[5] and (at - C.addressof(d.cons.contents)) % 16 == 0
    assert (rc.blocks[0].kind, rc.blocks[0].cons_len) == (2, len(t["rc"]["blocks"][0][1])) and C.string_at(C.addressof(rc.cons.contents) + rc.blocks[0].cons_off, rc.blocks[0].cons_len) == t["rc"]["blocks"][0][1]
    assert [d2.members[m].n_subs for m in range(1)] == [int(t["redetached"]["counts"][0][0])]


# ---------------------------------------------------------------- the kernels on the host
def test_close_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_close_idx.h on every named case of tests/close_gen.py (dumped to a file each, held against host_close's expectation and a scalar
    construction) and on random instances: validation, every kernel (the scans, the two stages, the chain, the ranks, the descriptors, the node rewrite, the list
    copies and the letter gather of pga_assemble_idx.h) against a direct scalar construction, every refusal of the host and of the kernels,
    and pga_rc_detach_args."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "close_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "close_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    files = []
    for name in cg.CASES:                                                        # every named case goes through the emulated kernels as a file
        files.append(str(tmp_path / f"{name}.bin"))
        cg.dump(cg.case(name), files[-1])
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith(f"close_emu OK ({len(cg.CASES)} named cases") and not noise, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------- self_merge_round(close=stand-in): the tables and the reading back without a device
def _canon(g):
    edit = lambda e: {f: [tuple(x) for x in e[f]] for f in ("subs", "dels", "inss")}
    return {"paths": {p: dict(v, nodes=list(v["nodes"])) for p, v in g["paths"].items()}, "nodes": {n: dict(v, position=tuple(v["position"])) for n, v in g["nodes"].items()},
            "blocks": {b: {"consensus": v["consensus"], "alignments": {n: edit(e) for n, e in v["alignments"].items()}} for b, v in g["blocks"].items()}}


def _round(run):
    from pangraph_amd.assemble import MergeError
    try:
        return _canon(run())
    except MergeError:
        return "MergeError"


def fake_reconsensus(blocks):
    """stands in for reconsensus.reconsensus: the kind follows the depth; a kind-1 block gets another first letter, a kind-2 block one more
    letter, and its last member (of two or more) comes back without an aligned position"""
    res = []
    for cons, members in blocks:
        kind = len(members) % 3 if cons else 0
        edits = [dict(e) for e in members]
        new = cons if kind == 0 else ("T" if cons[0] != "T" else "G") + cons[1:] + ("A" if kind == 2 else "")
        if kind == 2 and len(members) >= 2:
            edits[-1] = {"subs": [], "dels": [(0, len(new))], "inss": [(0, "ACGTAC")]}
        res.append((kind, new, edits, cg.edit(), [0] * len(members)))
    return res


def test_stand_in_close_against_the_tail_in_dicts(oracle_lib):
    import json

    import apply_gen as ag
    import promise_ref as pr
    import reweave_gen as rg
    import reweave_ref as rr
    from conftest import GOLDEN
    vec = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
    solve = lambda promises: [pr.solve_promise(oracle_lib.dll, q) for q in promises]
    calls = []

    def stand_in(t, flags):
        calls.append((flags, len(t["upd"]), len(t["detached"]["orphans"]), len(t["redetached"]["orphans"])))
        cl.Tables(t)                                                             # (the tables pack)
        return cg.flat_close(t, flags)

    def merged_round_is_merge_round(make, thr):
        """close._host_merge restates assemble.merge_round(blocks=None) to learn the merged ids: the two give the same graph, and the ids
        are the blocks the round made that hold members of two blocks before or are named by a promise"""
        from pangraph_amd import assemble as asm
        kw = dict(plan=rr.expected_call, slicer=ag.ref_slicer)
        g0, matches = make()
        g1, _ = make()
        before = set(g0["blocks"])
        want = _round(lambda: asm.merge_round(g0, matches, thr, solve, **kw))
        ids = []
        got = _round(lambda: (lambda r: ids.extend(r[1]) or r[0])(cl._host_merge(g1, matches, thr, solve, None, **kw)))
        assert got == want
        if want != "MergeError":
            assert ids == sorted(ids) and all(b in want["blocks"] and b not in before for b in ids)
        return ids

    def both(make, thr):
        kw = dict(plan=rr.expected_call, slicer=ag.ref_slicer, detach=dr.expected_call, rc=fake_reconsensus)
        g0, matches = make()
        g1, _ = make()
        want = _round(lambda: cl.self_merge_round(g0, matches, thr, solve=solve, **kw))
        got = _round(lambda: cl.self_merge_round(g1, matches, thr, close=stand_in, solve=solve, **kw))
        assert got == want
        return want

    assert len(merged_round_is_merge_round(lambda: rg.reference_graph(vec), vec["reweave"]["thr_len"])) >= 1
    assert sum(len(merged_round_is_merge_round(lambda: ag.random_graph(seed), rg.THR)) for seed in range(40)) >= 6
    want = both(lambda: rg.reference_graph(vec), vec["reweave"]["thr_len"])
    assert want != "MergeError" and len(calls) == 1 and calls[0][1] >= 1
    done = [both(lambda: ag.random_graph(seed), rg.THR) != "MergeError" for seed in range(40)]
    assert sum(done) >= 6 and len(calls) == 1 + sum(done)
    assert sum(c[3] for c in calls) >= 3                                         # (second-stage orphans went through the tables)
