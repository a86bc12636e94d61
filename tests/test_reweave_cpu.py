"""The front half of reweave without a GPU: the restatement tests/reweave_ref.py against the reference's own unit-test values
(tests/golden/reweave_vectors.json), XXH64 on the 24- and 48-byte streams, the host side of pangraph_amd/reweave.py against the header and
the restatement, the kernels of pga_reweave_idx.h in a stand-alone program under the host sanitizers (tests/emu/reweave_emu.cpp), and what
the GPU tests rely on their generated levels for."""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess

import pytest

import detach_ref as dr
import reweave_gen as rg
import reweave_ref as rr
from conftest import GOLDEN, ROOT
from pangraph_amd import batch
from pangraph_amd import reweave as rw

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
cg = rr.parse_cigar


# ---------------------------------------------------------------- cigar.rs
def test_invert_and_switch_vectors():
    assert rr.invert_cigar(cg(VEC["invert_cigar"]["cigar"])) == cg(VEC["invert_cigar"]["expected"])
    assert rr.cigar_switch_ref_qry(cg(VEC["switch_ref_qry"]["cigar"])) == cg(VEC["switch_ref_qry"]["expected"])
    with pytest.raises(rr.Err, match="unsupported operation kind"):
        rr.cigar_switch_ref_qry(cg(VEC["switch_ref_qry_unsupported"]["cigar"]))


@pytest.mark.parametrize("v", VEC["add_flanking_indel"], ids=lambda v: v["name"])
def test_add_flanking_indel_vectors(v):
    assert rr.add_flanking_indel(cg(v["cigar"]), v["kind"], v["add"], v["side"]) == cg(v["expected"])


@pytest.mark.parametrize("v", VEC["update_cigar"], ids=lambda v: v["name"])
def test_update_cigar_vectors(v):
    assert rr.update_cigar(cg(v["cigar"]), tuple(v["anchor"]), tuple(v["append"]), v["reverse"]) == cg(v["expected"])
    assert (v["cigar"], tuple(v["anchor"]), tuple(v["append"]), v["reverse"], v["expected"]) in rg.UPDATE_CIGAR_CASES


# ---------------------------------------------------------------- pangraph_interval.rs
def _hits(v):
    return [{"hit": {"name": v["block_id"], "start": h["start"], "end": h["end"]}, "new_block_id": h["new_block_id"], "is_anchor": h["is_anchor"],
             "reverse": h["reverse"], "cigar": None} for h in v["hits"]]


def test_create_and_refine_intervals_vectors():
    v = VEC["intervals"]
    created = rr.create_intervals(_hits(v), v["block_length"])
    assert [(i["start"], i["end"], i["new_block_id"]) for i in created] == \
        [(s, e, rr.gap_id(v["block_id"], s, e) if nb is None else nb) for s, e, nb in v["created"]]
    assert [i["aligned"] for i in created] == [nb is not None for _, _, nb in v["created"]]
    refined = rr.extract_intervals(_hits(v), v["block_length"], v["thr_len"])
    want = [(x["start"], x["end"], rr.gap_id(v["block_id"], x["start"], x["end"]) if x["new_block_id"] is None else x["new_block_id"], x["extend_left"], x["extend_right"])
            for x in v["refined"]]
    assert [(i["start"], i["end"], i["new_block_id"], i["extend_left"], i["extend_right"]) for i in refined] == want


# ---------------------------------------------------------------- reweave.rs
def _aln(a):
    return {"qry": dict(a["qry"]), "reff": dict(a["reff"]), "reverse": a["reverse"], "cigar": cg(a["cigar"]), "new_block_id": a.get("new_block_id"),
            "anchor_block": a.get("anchor_block")}


def test_extract_hits_vector():
    v = VEC["extract_hits"]
    got = rr.extract_hits(v["bid"], [_aln(a) for a in v["alignments"]])
    assert got == [{"hit": e["hit"], "new_block_id": e["new_block_id"], "is_anchor": e["is_anchor"], "reverse": e["reverse"],
                    "cigar": None if e["cigar"] is None else cg(e["cigar"])} for e in v["expected"]]


def test_group_promises_vector():
    v = VEC["group_promises"]
    h = [{"block_id": t["block_id"], "slice": t["consensus"], "is_anchor": t["is_anchor"], "reverse": t["reverse"],
          "cigar": None if t["cigar"] is None else cg(t["cigar"]), "extension": (None, None)} for t in v["to_merge"]]
    assert [(p["anchor"], p["append"], p["reverse"], p["cigar"]) for p in rr.group_promises(h)] == \
        [(e["anchor"], e["append"], e["reverse"], cg(e["cigar"])) for e in v["expected"]]


def test_assign_anchor_block_and_target_blocks_vectors():
    v = VEC["assign_anchor_block"]
    blocks = {int(b): {"consensus": v["consensus"][b], "depth": d} for b, d in v["depths"].items()}
    hit = lambda b: {"name": b, "start": 0, "end": 0}
    mergers = [{"qry": hit(q), "reff": hit(r), "reverse": True, "cigar": [], "new_block_id": None, "anchor_block": None} for q, r in v["alignments"]]
    rr.assign_anchor_block(mergers, blocks)
    assert [m["anchor_block"] for m in mergers] == v["expected"]
    t = VEC["target_blocks"]
    mergers = [{"qry": hit(q), "reff": hit(r), "k": k} for k, (q, r) in enumerate(t["alignments"])]
    assert [(bid, [m["k"] for m in ms]) for bid, ms in rr.target_blocks(mergers)] == [(int(b), ks) for b, ks in sorted(t["expected"].items(), key=lambda x: int(x[0]))]


@pytest.mark.parametrize("v", VEC["anchor_cases"], ids=lambda v: v["name"])
def test_anchor_case_vectors(v):
    blocks = {1: {"consensus": v["b1"][0], "depth": v["b1"][1]}, 2: {"consensus": v["b2"][0], "depth": v["b2"][1]}}
    m = [{"qry": {"name": v["qry"], "start": v["qry_interval"][0], "end": v["qry_interval"][1]},
          "reff": {"name": v["ref"], "start": v["ref_interval"][0], "end": v["ref_interval"][1]}, "reverse": False, "cigar": [], "new_block_id": None, "anchor_block": None}]
    rr.assign_anchor_block(m, blocks)
    assert m[0]["anchor_block"] == v["expected"]
    k = [c["name"] for c in VEC["anchor_cases"]].index(v["name"])
    assert rg.ANCHOR_CASES[k] == ((v["b1"][0], v["b1"][1]), (v["b2"][0], v["b2"][1]), (v["qry"], tuple(v["qry_interval"]), v["ref"], tuple(v["ref_interval"])), v["expected"])


def test_split_block_vector():
    v = VEC["split_block"]
    blocks = {v["bid"]: {"consensus": "A" * v["cons_len"], "depth": 3}}
    intervals, h = rr.split_block(v["bid"], [_aln(a) for a in v["alignments"]], blocks, v["thr_len"])
    assert [[i["start"], i["end"], i["aligned"]] for i in intervals] == v["expected_intervals"]
    assert [(t["block_id"], t["is_anchor"], t["reverse"], t["cigar"], list(t["slice"][1:])) for t in h] == \
        [(e["block_id"], e["is_anchor"], e["reverse"], None if e["cigar"] is None else cg(e["cigar"]), e["slice"]) for e in v["expected_to_merge"]]


def _reweave_vector():
    v = VEC["reweave"]
    blocks = {int(b): {"consensus": "ACGT" * (ln // 4) + "A" * (ln % 4), "depth": d} for b, (ln, d) in v["blocks"].items()}
    return v, blocks, [_aln(a) for a in v["alignments"]]


def test_reweave_vector_structure():
    v, blocks, mergers = _reweave_vector()
    counts, u, promises = rr.reweave_plan(mergers, blocks, v["thr_len"])
    ids = [m["new_block_id"] for m in mergers]
    assert ids == [rr.match_id(m["qry"], m["reff"]) for m in mergers] and len(set(ids)) == 4
    got = {p["new_block_id"]: p for p in promises}
    assert [p["new_block_id"] for p in promises] == sorted(ids)
    for e in v["expected_promises"]:
        p = got[ids[e["match"]]]
        assert (list(p["anchor"]), list(p["append"]), p["reverse"], p["cigar"]) == (e["anchor"], e["append"], e["reverse"], cg(e["cigar"]))
    unaligned = {str(bid): [[i["start"], i["end"]] for i in ivs if not i["aligned"]] for bid, ivs in u}
    assert {b: x for b, x in unaligned.items() if x} == v["expected_unaligned"]
    for bid, ivs in u:
        assert ivs[0]["start"] == 0 and ivs[-1]["end"] == len(blocks[bid]["consensus"])


# ---------------------------------------------------------------- the ids
def test_xxh64_on_the_id_streams():
    assert dr.xxh64(b"") == 0xEF46DB3751D8E999 and dr.xxh64(b"a") == 0xD24EC4F1A98C6E5B
    # (BlockId(7), Interval { start: 3, end: 11 }): three usize, little-endian -- 24 bytes, no stripe, three 8-byte steps
    stream = bytes([7, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0, 11, 0, 0, 0, 0, 0, 0, 0])
    assert struct.pack("<3Q", 7, 3, 11) == stream and rr.gap_id(7, 3, 11) == dr.xxh64(stream)
    # (&qry.name, &qry.interval, &reff.name, &reff.interval): 48 bytes, one stripe of 32 and two 8-byte steps
    q, r = {"name": 10, "start": 10, "end": 200}, {"name": 40, "start": 10, "end": 200}
    assert rr.match_id(q, r) == dr.xxh64(struct.pack("<6Q", 10, 10, 200, 40, 10, 200)) != rr.match_id(r, q)
    from pangraph_amd import detach as dt
    for words in ((0,) * 6, ((1 << 64) - 1,) * 6, (1, 2, 3, 4, 5, 6)):
        assert dt.xxh64(struct.pack("<6Q", *words)) == dr.xxh64(struct.pack("<6Q", *words))
        assert dt.xxh64(struct.pack("<3Q", *words[:3])) == dr.xxh64(struct.pack("<3Q", *words[:3]))


# ---------------------------------------------------------------- the C interface
def test_plan_structs_match_the_header(tmp_path):
    pairs = [("pga_plan_block_t", rw.plan_block_t), ("pga_plan_match_t", rw.plan_match_t), ("pga_plan_block_res_t", rw.plan_block_res_t),
             ("pga_plan_interval_t", rw.plan_interval_t), ("pga_plan_promise_t", rw.plan_promise_t), ("pga_plan_counters_t", rw.plan_counters_t),
             ("pga_plan_out_t", rw.plan_out_t), ("pga_match_t", batch.pga_match_t)]
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


def test_library_exports_the_plan_entries(product_so):
    out = subprocess.run(["nm", "-D", "--defined-only", product_so], check=True, capture_output=True, text=True).stdout
    assert {"pga_plan_merge", "pga_plan_free"} <= set(line.split()[-1] for line in out.splitlines() if " T " in line)


def test_packed_level_is_what_the_restatement_reads():
    groups, matches = rg.random_level(3)
    K = rw._Packed(groups, matches)
    flat = [b for g in groups for b in g]
    assert [K.off[i] for i in range(len(groups) + 1)] == [sum(len(g) for g in groups[:i]) for i in range(len(groups) + 1)]
    assert [(K.B[i].block_id, K.B[i].cons_len, K.B[i].depth, K.B[i].consensus.decode()) for i in range(len(flat))] == \
        [(b["block_id"], len(b["consensus"]), b["depth"], b["consensus"]) for b in flat]
    for i, m in enumerate(matches):
        r = K.M[i]
        assert (r.group, r.qry, r.ref, r.qry_start, r.qry_end, r.ref_start, r.ref_end, r.reverse) == \
            (m["group"], m["qry"], m["ref"], m["qry_start"], m["qry_end"], m["ref_start"], m["ref_end"], int(m["reverse"]))
        assert rr.unpack_cigar([K.G[r.cigar_off + k] for k in range(r.n_cigar)]) == m["cigar"]
    assert rw.pack_cigar([("M", 3), ("X", 1)]) == rr.pack_cigar([("M", 3), ("X", 1)]) == [3 << 4, 1 << 4 | 8]


def test_kernels_under_emulation_and_sanitizers(tmp_path):
    """pga_reweave_idx.h: the host tables and every kernel, std sorts and loops standing in for rocPRIM, on the edge level (1, 2, 63, 64, 65
    hits on a block; CIGARs of 1 .. 3001 operations with all four flanks) and on 18 random levels, with and without a bit plane, against a
    direct scalar construction; XXH64 of 3 and 6 words against the byte-stream implementation."""
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "reweave_emu")
    subprocess.run([cxx, "-std=c++17", "-g1", "-O1", "-DPGA_EMU", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "emu", "reweave_emu.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    noise = [ln for ln in r.stderr.splitlines() if ln and "doesn't fully support makecontext/swapcontext" not in ln]
    assert r.returncode == 0 and r.stdout.startswith("reweave_emu OK") and not noise, (r.returncode, r.stdout, r.stderr)


# ---------------------------------------------------------------- what the GPU tests rely on
def _exts(e):
    return [(i["extend_left"], i["extend_right"]) for i in e["intervals"]]


def test_generated_levels_hold_what_the_gpu_tests_need():
    groups, matches = rg.hits_level()
    e = rr.expected_call(groups, matches, rg.THR)
    per_block = {}
    for m in matches:
        for side in ("qry", "ref"):
            per_block[(m["group"], m[side])] = per_block.get((m["group"], m[side]), 0) + 1
    assert set(rg.HIT_COUNTS) <= set(per_block.values()) and e["n_failed"] == 0
    assert len(e["intervals"]) > 256 and len(matches) > 256 and any(not any(m["group"] == g for m in matches) for g in range(len(groups)))
    assert [b["block_id"] for b in groups[0]] == [b["block_id"] for b in groups[2]][:len(groups[0])]
    assert [b["block"] for b in e["blocks"][:3]] != sorted(b["block"] for b in e["blocks"][:3])          # the output order is by block id, not by input index
    for (g, m), n in zip(rg.promise_levels(), (63, 64, 65)):
        assert len(rr.expected_call(g, m, rg.THR)["promises"]) == n
    # refinement: every rule on blocks that succeed
    groups, matches = rg.refine_level()
    e = rr.expected_call(groups, matches, rg.THR)
    s = rg.THR - 1
    assert e["n_failed"] == 0
    x = _exts(e)
    assert (s, 0) in x and (0, s) in x and (1, s) in x and (1, 1) in x and (0, 1) in x                   # start / end / both on one hit / a one-letter gap left
    assert any(not i["aligned"] and i["end"] - i["start"] == rg.THR for i in e["intervals"])            # a gap of exactly thr_len stays
    assert e["counters"]["intervals_before"] > e["counters"]["intervals_after"]
    assert rr.expected_call(groups, matches, 0)["counters"]["intervals_before"] == rr.expected_call(groups, matches, 0)["counters"]["intervals_after"]
    # failing blocks: the codes a block can report
    codes = {}
    for name, layouts in rg.failing_blocks().items():
        L = rg.Level(5)
        L.group(layouts)
        e = rr.expected_call(*L.level(), rg.THR)
        failed = [b for b in e["blocks"] if b["status"]]
        assert len(failed) == 1 and e["intervals"] is None and e["promises"] is None and e["cigars"] is None
        codes[name] = (failed[0]["status"], failed[0]["fail_interval"], failed[0]["block"])
    assert codes == {"short_hit": (1, 1, 0), "short_hit_first": (1, 0, 0), "gap_before_short_hit": (5, 0, 0), "gap_between": (5, 1, 0),
                     "gap_behind_short_hit": (1, 2, 0), "short_hit_then_trailing": (1, 2, 0), "later_block": (1, 2, 1)}
    # CIGARs: lengths, both orientations, both anchors, flanks that lengthen and flanks that insert
    groups, matches = rg.cigar_level()
    e = rr.expected_call(groups, matches, rg.THR)
    assert e["n_failed"] == 0 and {len(m["cigar"]) for m in matches} >= set(rg.CIGAR_LENGTHS) | {0}
    grown = [p["n_cigar"] - len(matches[p["match"]]["cigar"]) for p in e["promises"]]
    assert set(grown) == {0, 1, 2, 3, 4}
    assert {(m["reverse"], e["matches"][k]["anchor"]) for k, m in enumerate(matches)} == {(False, 0), (False, 1), (True, 0), (True, 1)}
    # the anchor decision: every route, with and without a batch
    groups, matches = rg.anchor_level()
    a, b = rr.expected_call(groups, matches, rg.THR, resident=False), rr.expected_call(groups, matches, rg.THR, resident=True)
    assert [(m["anchor"], m["ref_n"], m["qry_n"]) for m in a["matches"]] == [(m["anchor"], m["ref_n"], m["qry_n"]) for m in b["matches"]]
    assert a["counters"]["by_mask"] == 0 and b["counters"]["by_mask"] > 5 and b["counters"]["by_letters"] > 5 and b["counters"]["by_depth"] == 2
    assert {m["anchor"] for m in b["matches"] if m["route"] == 2} == {0, 1}
    assert any(m["route"] == 2 and m["ref_n"] == 0 and m["qry_n"] == 0 for m in b["matches"])            # R / Y / n: masked, no N
    last = matches[-1]
    assert last["qry_end"] == len(groups[-1][last["qry"]]["consensus"]) and last["qry"] == len(groups[-1]) - 1
    e = rr.expected_call(*rg.anchor_cases_level(), 1)
    assert [("ref", "qry")[m["anchor"]] for m in e["matches"]] == [c[3] for c in rg.ANCHOR_CASES]


def test_no_block_can_report_code_3():
    """check_interval_conditions' code 3 (the left neighbour is short) needs a short aligned interval in front of a short gap; that interval is
    visited first and fails with code 1.  Codes 2 and 4 need two gaps in a row.  Over every layout of up to four pieces with lengths around
    thr_len, the restatement never raises them."""
    import itertools
    thr, seen = 5, set()
    for n in range(1, 5):
        for kinds in itertools.product("gh", repeat=n):
            if "h" not in kinds or any(a == b == "g" for a, b in zip(kinds, kinds[1:])):
                continue
            for lens in itertools.product((1, thr - 1, thr, thr + 2), repeat=n):
                hits, at = [], 0
                for k, ln in zip(kinds, lens):
                    if k == "h":
                        hits.append({"hit": {"name": 1, "start": at, "end": at + ln}, "new_block_id": at, "is_anchor": True, "reverse": False, "cigar": []})
                    at += ln
                try:
                    rr.extract_intervals(hits, at, thr)
                    seen.add(0)
                except rr.Err as e:
                    seen.add(e.code)
    assert seen == {0, 1, 5}


# ---------------------------------------------------------------- the graph level, the restatements standing in for the device
def test_reweave_graph_level_on_the_reference_example():
    """test_reweave (reweave.rs:872-1137): path lengths, node positions and strands, which nodes share a block, which blocks are in the graph
    and which in a promise, the sliced edit of node 200/3 -- pangraph_amd.reweave.reweave over reweave_ref and slice_ref"""
    import slice_ref as sr
    v, w = VEC["reweave"], VEC["reweave_graph"]
    E = rg.edit_from_json
    g, matches = rg.reference_graph(VEC)
    slicer = lambda bl: sr.slice_blocks([dict(b, intervals=[sr.interval(s, e, bool(f), False, bool(f)) for s, e, f in b["intervals"]]) for b in bl])
    g, promises = rw.reweave(g, matches, v["thr_len"], plan=rr.expected_call, slicer=slicer)
    node = lambda ref: g["nodes"][g["paths"][int(ref[0])]["nodes"][ref[1]]]
    for p in w["paths"]:
        nodes = [g["nodes"][n] for n in g["paths"][int(p)]["nodes"]]
        assert len(nodes) == w["expected_path_lengths"][p]
        assert [list(n["position"]) for n in nodes] == w["expected_positions"][p] and "".join(n["strand"] for n in nodes) == w["expected_strands"][p]
        assert all(n["path_id"] == int(p) for n in nodes)
    for a, b in w["same_block"]:
        assert node(a)["block_id"] == node(b)["block_id"]
    anchors = {id(q["anchor"]): q for q in promises}
    assert len(promises) == 4 and set(g["blocks"]) & {q["new_block_id"] for q in promises} == set()
    for ref in w["in_graph"]:
        nid = g["paths"][int(ref[0])]["nodes"][ref[1]]
        assert g["blocks"][node(ref)["block_id"]]["alignments"][nid] == E(w["expected_edit_200_3"])
    for ref in w["in_promise_anchor"]:
        assert node(ref)["block_id"] in {q["new_block_id"] for q in promises} and node(ref)["block_id"] not in g["blocks"]
    assert not set(g["blocks"]) & {10, 20, 30, 40, 50} and all(n["block_id"] in g["blocks"] or n["block_id"] in {q["new_block_id"] for q in promises} for n in g["nodes"].values())
    by_id = {q["new_block_id"]: q for q in promises}
    for e, q in zip(v["expected_promises"], [by_id[rr.match_id({"name": a["qry"]["name"], "start": a["qry"]["start"], "end": a["qry"]["end"]},
                                                                 {"name": a["reff"]["name"], "start": a["reff"]["start"], "end": a["reff"]["end"]})] for a in v["alignments"]]):
        assert q["cigar"] == cg(e["cigar"]) and q["reverse"] == e["reverse"]
        assert len(q["anchor"]["consensus"]) == e["anchor"][2] - e["anchor"][1] and len(q["append"]["consensus"]) == e["append"][2] - e["append"][1]
        assert set(q["anchor"]["alignments"]) | set(q["append"]["alignments"]) <= set(g["nodes"])
    # a threshold above the shortest hits: the first failing block in BTreeMap order speaks, with the reference's code and interval
    with pytest.raises(rw.ReweaveError) as err:
        rw.reweave(rg.reference_graph(VEC)[0], matches, 150, plan=rr.expected_call, slicer=slicer)
    assert str(err.value) == "block 20: refine_intervals fails with code 5 at interval 1"
