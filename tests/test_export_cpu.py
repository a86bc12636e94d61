"""The restatement of export block-sequences / export core-genome (tests/export_ref.py) against the reference's own vectors
(tests/golden/export_vectors.json) and against a graph the reference wrote (tests/golden/plasmids.json.gz spells
tests/golden/plasmids.fa.gz); the JSON loader of pangraph_amd.export; the aligned run builder (pga_runs.h) in a stand-alone host program under the address and undefined-behaviour sanitizers.  No GPU."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

import export_ref as er
import mapvarbind as mb
import promise_ref as pr
import reconstruct_ref as rr
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def vectors():
    return json.load(open(os.path.join(GOLDEN, "export_vectors.json")))


@pytest.fixture(scope="module")
def plasmids():
    from pangraph_amd.export import core_from_json
    from pangraph_amd.reconstruct import graph_from_json
    raw = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz"), "rt"))
    blocks, paths, names = graph_from_json(raw)
    args, keys, order = core_from_json(raw, names[0])
    return raw, blocks, paths, names, args, keys, order


# ---------------------------------------------------------------- the reference's vectors
def test_core_block_aln_general_case(vectors):
    from pangraph_amd.export import core_from_json
    case = vectors["core_block_aln_general_case"]
    assert len(case["expected"]) == 4
    for exp in case["expected"]:
        args, keys, order = core_from_json(case["graph"], exp["guide"])
        assert keys == ["Path A", "Path B"] and args["n_paths"] == 2 and args["member_path"] == [0, 1, 0, 1, 1]
        got = er.core_block_aln(args["blocks"], args["member_path"], keys, args["guide_path"], args["guide_nodes"], exp["aligned"])
        assert got == [tuple(r) for r in exp["records"]]
        rows, core = er.expected_results(aligned=exp["aligned"], **args)
        assert [(k, r["seq"]) for k, r in zip(keys, order(rows))] == got and all(r["status"] == 0 for r in rows)
        assert [c["block"] for c in core] == ([0, 1] if exp["guide"] == "Path A" else [1, 0])          # block 3 (index 2) is not core
        assert [c["reverse"] for c in core] == ([False, True] if exp["guide"] == "Path A" else [False, True]) and [c["col"] for c in core] == [0, 20]


def test_concatenate_records_vectors(vectors):
    assert [c["name"] for c in vectors["concatenate_records"]] == ["general_case", "single_entry", "multiple_entries_same_name"]
    for c in vectors["concatenate_records"]:
        assert er.concatenate_records([[tuple(r) for r in entries] for entries in c["input"]]) == [tuple(r) for r in c["expected"]]
    bad = vectors["concatenate_records_error"]
    with pytest.raises(er.ExportError) as e:
        er.concatenate_records([[tuple(r) for r in entries] for entries in bad["input"]])
    assert str(e.value) == bad["error"]
    assert er.concatenate_records([]) == []


def test_reverse_complement_keeps_the_gap(vectors):
    assert vectors["reverse_complement"] == [["N-", "-N"]]
    for src, exp in vectors["reverse_complement"]:
        assert pr.reverse_complement(src) == exp


def test_apply_aligned_rules():
    E = lambda **k: {"subs": k.get("subs", []), "dels": k.get("dels", []), "inss": k.get("inss", [])}
    assert er.apply_aligned("ACGTACGT", E(subs=[(1, "T"), (1, "G")])) == "AGGTACGT"                      # the later of two wins
    assert er.apply_aligned("ACGTACGT", E(subs=[(3, "A")], dels=[(2, 3), (3, 3)])) == "AC----GT"        # lost under overlapping deletions
    assert er.apply_aligned("ACGTACGT", E(inss=[(0, "TTT"), (8, "GG")])) == "ACGTACGT"                   # insertions are missing
    assert er.apply_aligned("AC-T", E(subs=[(0, "-")])) == "-C-T"                                       # a literal '-' is kept
    assert er.apply_aligned("ACGT", E(dels=[(0, 4)])) == "----"
    blocks = [{"consensus": "AC-TX", "members": [E(), E(dels=[(2, 1)]), E(dels=[(2, 1), (4, 1)])]}]
    assert [r["status"] for r in er.expected_block_sequences(blocks, aligned=False)] == [3, 0, 0]
    assert [r["status"] for r in er.expected_block_sequences(blocks, aligned=True)] == [0, 0, 0]
    rows, core = er.expected_results(blocks, [0, 1, 2], 3, 0, [(0, 0, True)], aligned=True)
    assert [r["status"] for r in rows] == [2, 2, 0] and rows[2]["seq"] == "-A-GT" and core == [dict(block=0, reverse=True, col=0, cons_len=5)]
    rows, _ = er.expected_results(blocks, [0, 1, 2], 3, 0, [(0, 0, True)], aligned=False)
    assert [(r["status"], r["len"]) for r in rows] == [(2, 5), (2, 4), (0, 3)]                          # 2 before 3
    with pytest.raises(er.CallFailure, match="not named"):
        er.expected_results(blocks, [0, 1, 2], 3, 0, [])
    with pytest.raises(er.CallFailure, match="twice"):
        er.expected_results(blocks, [0, 1, 2], 3, 0, [(0, 0, False), (0, 0, True)])
    with pytest.raises(er.CallFailure, match="not on guide_path"):
        er.expected_results(blocks, [0, 1, 2], 3, 0, [(0, 1, False)])


# ---------------------------------------------------------------- the plasmid graph
CORE_LEN = 64989


def test_unaligned_block_sequences_spell_the_plasmids(plasmids):
    raw, blocks, paths, names, args, keys, _ = plasmids
    by_name = dict(zip(*rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))))
    recs = [er.sequences(b, [None] * len(b["members"]), False) for b in blocks]
    assert sum(len(r) for r in recs) == 1042 and keys == names
    for p, name in zip(paths, names):
        genome = "".join(pr.reverse_complement(recs[b][m][1]) if rev else recs[b][m][1] for b, m, rev in p["nodes"])
        assert rr.rotate_right(genome, p["first_pos"]) == by_name[name]
    rows = er.expected_block_sequences(blocks, aligned=False)
    assert [r["seq"] for r in rows] == [s for r in recs for _, s in r] and all(r["status"] == 0 for r in rows)


def test_plasmid_core_alignment(plasmids):
    """27 core blocks over the 15 paths; their consensus lengths sum to 64 989, the alignment length the reference's own tests assert
    on this file (packages/pypangraph/tests/test_graph.py:108, test_alignments.py:70) -- not the 64 983 of the issue that asked for this
    test, which no count of the graph gives.  None of the 15 paths reads a core block in reverse; the reverse reading is checked on the
    walk of a path along its other strand (nodes in reverse order, strands flipped)."""
    from pangraph_amd.export import core_from_json
    raw, blocks, paths, names, args, keys, _ = plasmids
    first = er.member_first(blocks)
    core_ids = er.core_block_ids(blocks, args["member_path"], 15)
    assert len(core_ids) == 27 and sum(len(blocks[b]["consensus"]) for b in core_ids) == CORE_LEN
    no_ins = lambda e: {"subs": e["subs"], "dels": e["dels"], "inss": []}
    for b in blocks:                                                      # every block-sequence row
        for (_, aln), e in zip(er.sequences(b, [None] * len(b["members"]), True), b["members"]):
            assert len(aln) == len(b["consensus"]) and aln.replace("-", "") == mb.apply_edit(b["consensus"], no_ins(e))
    reversed_somewhere = 0
    for guide in names:
        a, k, order = core_from_json(raw, guide)
        assert a["member_path"] == args["member_path"] and k == keys
        rows, core = er.expected_results(aligned=True, **a)
        assert len(rows) == 15 and all(r["status"] == 0 and r["len"] == CORE_LEN for r in rows)
        assert sorted(c["block"] for c in core) == core_ids and [c["col"] for c in core] == [sum(x["cons_len"] for x in core[:i]) for i in range(27)]
        reversed_somewhere += any(c["reverse"] for c in core)
        for p, r in enumerate(rows):
            parts = []
            for c in core:
                j = a["member_path"][first[c["block"]]:first[c["block"] + 1]].index(p)
                s = mb.apply_edit(blocks[c["block"]]["consensus"], no_ins(blocks[c["block"]]["members"][j]))
                parts.append(pr.reverse_complement(s) if c["reverse"] else s)
            assert r["seq"].replace("-", "") == "".join(parts)
        assert [x["seq"] for x in order(rows)] == [s for _, s in er.core_block_aln(a["blocks"], a["member_path"], k, a["guide_path"], a["guide_nodes"], True)]
    assert reversed_somewhere == 0
    a, k, order = core_from_json(raw, names[4])
    a["guide_nodes"] = [(b, m, not rev) for b, m, rev in reversed(a["guide_nodes"])]
    rows, core = er.expected_results(aligned=True, **a)
    fwd, fwd_core = er.expected_results(aligned=True, **core_from_json(raw, names[4])[0])
    assert all(c["reverse"] for c in core) and [c["block"] for c in core] == [c["block"] for c in reversed(fwd_core)]
    assert [r["seq"] for r in rows] == [pr.reverse_complement(r["seq"]) for r in fwd]


# ---------------------------------------------------------------- the aligned run builder
def test_aligned_run_builder_under_sanitizers(tmp_path):
    """dev/export_runs_check.cpp: aligned_segments and a scalar walk of its run tables against a direct apply_aligned, host code only"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host compiler")
    exe = str(tmp_path / "export_runs_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "pangraph_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "dev", "export_runs_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("export_runs_check OK") and not r.stderr, (r.returncode, r.stdout, r.stderr)
