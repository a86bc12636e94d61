"""pga_block_sequences and pga_core_alignment (export block-sequences and export core-genome on the device, streamed through a sink:
k_export_rows, pga_export_rows.h / pga_export.hip) against the restatement tests/export_ref.py, the reference's own vectors
(tests/golden/export_vectors.json) and a graph the reference wrote (tests/golden/plasmids.json.gz).  Every comparison is exact."""
import gzip
import json
import os
import random

import pytest

import export_gen as eg
import export_ref as er
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CORE_LEN = 64989
KNOBS = ("PGA_EXPORT_TILE_KB", "PGA_EXPORT_RUNS_KB")


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def both_entries(dll, a, aligned, order_rows=None, order_members=None, want_seqs=True):
    """both entries against export_ref; -> (block rows, core rows, core)"""
    from pangraph_amd.export import block_sequences, core_alignment
    got_b = block_sequences(a["blocks"], aligned, order_members, want_seqs, dll=dll)
    exp_b = er.expected_block_sequences(a["blocks"], aligned)
    got_r, got_core = core_alignment(aligned=aligned, order=order_rows, want_seqs=want_seqs, dll=dll, **a)
    exp_r, exp_core = er.expected_results(aligned=aligned, **a)
    if not want_seqs:
        exp_b = [dict(r, seq=None) for r in exp_b]; exp_r = [dict(r, seq=None) for r in exp_r]
    for what, got, exp in (("block", got_b, exp_b), ("core", got_r, exp_r)):
        assert len(got) == len(exp)
        for i, (g, e) in enumerate(zip(got, exp)):
            assert g == e, (what, aligned, i, g["status"], e["status"], g["len"], e["len"])
    assert got_core == exp_core
    return got_b, got_r, got_core


# ---------------------------------------------------------------- 1. the reference's vectors
def test_reference_vectors(gpu_lib):
    from pangraph_amd.export import core_alignment, core_from_json, core_records
    vectors = json.load(open(os.path.join(GOLDEN, "export_vectors.json")))
    case = vectors["core_block_aln_general_case"]
    assert len(case["expected"]) == 4
    for exp in case["expected"]:
        args, keys, in_record_order = core_from_json(case["graph"], exp["guide"])
        rows, core = core_alignment(aligned=exp["aligned"], dll=gpu_lib.dll, **args)
        assert [(k, r["seq"]) for k, r in zip(sorted(keys, key=str.encode), in_record_order(rows))] == [tuple(r) for r in exp["records"]]
        assert list(core_records(case["graph"], exp["guide"], exp["aligned"], dll=gpu_lib.dll)) == [tuple(r) for r in exp["records"]]
        for aligned in (True, False):
            both_entries(gpu_lib.dll, args, aligned)
    for src, want in vectors["reverse_complement"]:                       # "N-" -> "-N": one block, one path, read in reverse, aligned
        rows, _ = core_alignment([{"consensus": src, "members": [eg.E()]}], [0], 1, 0, [(0, 0, True)], dll=gpu_lib.dll)
        assert rows == [dict(status=0, len=len(src), seq=want)]


# ---------------------------------------------------------------- 2. the plasmid graph
@pytest.fixture(scope="module")
def plasmids():
    from pangraph_amd.export import core_from_json
    from pangraph_amd.reconstruct import graph_from_json
    raw = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz"), "rt"))
    blocks, paths, names = graph_from_json(raw)
    return raw, blocks, names


def test_plasmid_block_sequences(gpu_lib, plasmids):
    from pangraph_amd.export import block_sequences
    raw, blocks, names = plasmids
    got = block_sequences(blocks, aligned=False, dll=gpu_lib.dll)
    assert len(got) == 1042 and got == er.expected_block_sequences(blocks, aligned=False)


def test_plasmid_core_alignment(gpu_lib, plasmids):
    from pangraph_amd.export import core_alignment, core_from_json, core_records
    raw, blocks, names = plasmids
    a, keys, in_record_order = core_from_json(raw, names[4])
    rows, core = core_alignment(aligned=True, dll=gpu_lib.dll, **a)
    assert len(rows) == 15 and all(r["status"] == 0 and r["len"] == CORE_LEN == len(r["seq"]) for r in rows) and len(core) == 27
    want = er.core_block_aln(a["blocks"], a["member_path"], keys, a["guide_path"], a["guide_nodes"], True)
    assert [(k, r["seq"]) for k, r in zip(sorted(keys, key=str.encode), in_record_order(rows))] == want
    assert core == er.expected_results(aligned=True, **a)[1]
    assert list(core_records(raw, names[4], dll=gpu_lib.dll)) == want
    # the guide walked along its other strand: every piece is reverse
    a["guide_nodes"] = [(b, m, not rev) for b, m, rev in reversed(a["guide_nodes"])]
    rows, core = core_alignment(aligned=True, dll=gpu_lib.dll, **a)
    assert all(c["reverse"] for c in core) and len(core) == 27
    assert [(k, r["seq"]) for k, r in zip(sorted(keys, key=str.encode), in_record_order(rows))] == er.core_block_aln(a["blocks"], a["member_path"], keys, a["guide_path"], a["guide_nodes"], True)
    exp_rows, exp_core = er.expected_results(aligned=True, **a)
    assert rows == exp_rows and core == exp_core


# ---------------------------------------------------------------- 3. unit and tile edges
@pytest.mark.parametrize("tile_kb", ["4", None])
def test_unit_and_tile_edges(gpu_lib, monkeypatch, tile_kb):
    if tile_kb:
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", tile_kb)
    a = eg.edge_graph()
    for aligned in (True, False):
        got_b, got_r, core = both_entries(gpu_lib.dll, a, aligned)
        assert sorted({r["len"] for r in got_b[:24]} if aligned else {r["len"] for r in got_b[:24:3]}) == list(eg.UNIT_EDGE_LENGTHS)
        assert len(core) == len(a["blocks"]) and [c["block"] for c in core[:3]] == [1, 2, 0] and any(c["reverse"] for c in core)


# ---------------------------------------------------------------- 4. the knobs change no result
def test_knob_independence(gpu_lib, monkeypatch):
    from pangraph_amd.export import Collector, core_alignment_packed, block_sequences_packed
    from pangraph_amd.reconstruct import _Packed
    a = eg.big_graph()
    exp_rows, exp_core = er.expected_results(aligned=True, **a)
    exp_blocks = er.expected_block_sequences(a["blocks"], aligned=True)
    assert sum(r["len"] for r in exp_rows) > 290000
    K = _Packed(a["blocks"], [])
    guide = [(K.mem_first[b] + m, rev) for b, m, rev in a["guide_nodes"]]
    order = list(range(6)); random.Random(3).shuffle(order)
    for tile_kb, runs_kb in ((None, None), ("4", None), (None, "1"), ("4", "1")):
        for k, v in zip(KNOBS, (tile_kb, runs_kb)):
            monkeypatch.setenv(k, v) if v else monkeypatch.delenv(k, raising=False)
        sink = Collector()
        rows, core = core_alignment_packed(K, a["member_path"], 6, a["guide_path"], guide, True, order, dll=gpu_lib.dll, sink=sink)
        assert rows == exp_rows and core == exp_core, (tile_kb, runs_kb)
        assert eg.check_segments(sink, [r["len"] for r in rows]) == order
        if tile_kb:
            assert sink.tiles > 2 and sink.tiles >= sum(r["len"] for r in rows) // 4096
        sink = Collector()
        assert block_sequences_packed(K, True, dll=gpu_lib.dll, sink=sink) == exp_blocks, (tile_kb, runs_kb)
        assert eg.check_segments(sink, [r["len"] for r in exp_blocks]) == [m for m, r in enumerate(exp_blocks) if r["len"]]
        assert core_alignment_packed(K, a["member_path"], 6, a["guide_path"], guide, True, order, want_seqs=False, dll=gpu_lib.dll)[0] == [dict(r, seq=None) for r in exp_rows]


def test_knobs_are_checked(gpu_lib, monkeypatch):
    from pangraph_amd import batch
    from pangraph_amd.export import block_sequences
    blocks = [{"consensus": "ACGT", "members": [eg.E()]}]
    for k, v in (("PGA_EXPORT_TILE_KB", "6"), ("PGA_EXPORT_TILE_KB", "0"), ("PGA_EXPORT_RUNS_KB", "0"), ("PGA_EXPORT_TILE_KB", "big")):
        monkeypatch.setenv(k, v)
        with pytest.raises(batch.PgaError, match=k):
            block_sequences(blocks, dll=gpu_lib.dll)
        monkeypatch.delenv(k)
    assert block_sequences(blocks, dll=gpu_lib.dll) == [dict(status=0, len=4, seq="ACGT")]


# ---------------------------------------------------------------- 5. random graphs
SEEDS = list(range(40))


@pytest.mark.parametrize("seed", SEEDS)
def test_random_graphs(gpu_lib, monkeypatch, seed):
    a, order_rows, order_members = eg.random_graph(seed)
    if seed % 2:
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
    for aligned in (True, False):
        both_entries(gpu_lib.dll, a, aligned, order_rows, order_members)
        both_entries(gpu_lib.dll, a, aligned, order_rows, order_members, want_seqs=False)


# ---------------------------------------------------------------- 6. statuses and failures
def test_call_failures(gpu_lib):
    from pangraph_amd import batch
    from pangraph_amd.export import block_sequences, core_alignment
    blocks = [{"consensus": "AC-TX", "members": [eg.E(), eg.E(dels=[(2, 1)]), eg.E(dels=[(2, 1), (4, 1)])]}]
    good = dict(blocks=blocks, member_path=[0, 1, 2], n_paths=3, guide_path=0, guide_nodes=[(0, 0, True)])
    both_entries(gpu_lib.dll, good, True); both_entries(gpu_lib.dll, good, False)     # statuses 2 before 3 (test_apply_aligned_rules)

    def fails(match, **change):
        a = dict(good, **change)
        with pytest.raises(er.CallFailure):
            er.expected_results(**a)
        for want_seqs in (True, False):
            with pytest.raises(batch.PgaError, match=match) as e:
                core_alignment(want_seqs=want_seqs, dll=gpu_lib.dll, **a)
            assert str(e.value).startswith("pga_core_alignment: ")
    fails("not named", guide_nodes=[])
    fails("twice", guide_nodes=[(0, 0, False), (0, 0, True)])
    fails("not on guide_path", guide_nodes=[(0, 1, False)])
    fails("member that does not exist", guide_nodes=[(0, 3, False)])
    fails("member that does not exist", guide_nodes=[(1, 0, False)])
    fails("member_path names a path", member_path=[0, 1, 3])
    fails("guide_path names a path", guide_path=3)
    fails("guide_path names a path", guide_path=-1)
    for bad, match in ((eg.E(subs=[(5, "A")]), "substitution beyond"), (eg.E(subs=[(0, "Ā")]), "outside one byte"), (eg.E(dels=[(3, 3)]), "deletion beyond"),
                       (eg.E(inss=[(6, "A")]), "insertion beyond")):
        b2 = [{"consensus": "AC-TX", "members": [eg.E(), bad, eg.E()]}]
        fails(match, blocks=b2)
        with pytest.raises(er.CallFailure):
            er.expected_block_sequences(b2)
        for aligned in (True, False):
            with pytest.raises(batch.PgaError, match=match):
                block_sequences(b2, aligned, dll=gpu_lib.dll)
    for order in ([0, 0, 1], [0, 1, 3]):
        with pytest.raises(batch.PgaError, match="not a permutation"):
            core_alignment(order=order, dll=gpu_lib.dll, **good)
        with pytest.raises(batch.PgaError, match="not a permutation"):
            block_sequences(blocks, order=order, want_seqs=False, dll=gpu_lib.dll)


def test_row_over_2_31_letters_fails_the_call(gpu_lib):
    """three core blocks that share one consensus of 2^30 - 1 letters: the row would have more than 2^31; nothing is launched"""
    from pangraph_amd import batch
    from pangraph_amd.export import core_alignment_packed
    from pangraph_amd.reconstruct import _Packed
    cons = bytes((1 << 30) - 1)
    K = _Packed([{"consensus": cons, "members": [eg.E()]} for _ in range(3)], [])
    with pytest.raises(batch.PgaError, match="row over 2\\^31 letters"):
        core_alignment_packed(K, [0, 0, 0], 1, 0, [(0, False), (1, False), (2, True)], dll=gpu_lib.dll)


def test_empty_results_and_no_core(gpu_lib):
    from pangraph_amd.export import Collector, core_alignment, core_alignment_packed
    from pangraph_amd.reconstruct import _Packed
    blocks = [{"consensus": "ACGT", "members": [eg.E(), eg.E()]}, {"consensus": "TTTT", "members": [eg.E()]}]
    assert er.expected_results(blocks, [0, 0, 0], 0, 0, []) == ([], [])
    assert core_alignment(blocks, [0, 0, 0], 0, 0, [], dll=gpu_lib.dll) == ([], [])
    a = dict(blocks=blocks, member_path=[0, 0, 1], n_paths=2, guide_path=0, guide_nodes=[(0, 1, True), (0, 0, False)])   # no block is core
    exp = er.expected_results(**a)
    assert exp == ([dict(status=0, len=0, seq="")] * 2, [])
    sink = Collector()
    K = _Packed(blocks, [])
    assert core_alignment_packed(K, a["member_path"], 2, 0, [(1, True), (0, False)], dll=gpu_lib.dll, sink=sink) == exp and sink.tiles == 0
    assert core_alignment(want_seqs=False, dll=gpu_lib.dll, **a) == ([dict(status=0, len=0, seq=None)] * 2, [])


def test_sink_stops_the_export(gpu_lib, monkeypatch):
    from pangraph_amd import batch
    from pangraph_amd.export import Collector, core_alignment_packed
    from pangraph_amd.reconstruct import _Packed
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
    a = eg.big_graph(n_paths=3, n_blocks=8)
    exp = er.expected_results(aligned=True, **a)
    assert sum(r["len"] for r in exp[0]) > 5 * 4096
    K = _Packed(a["blocks"], [])
    guide = [(K.mem_first[b] + m, rev) for b, m, rev in a["guide_nodes"]]
    sink = Collector(stop_at=2)
    with pytest.raises(batch.PgaError, match="sink stopped the export"):
        core_alignment_packed(K, a["member_path"], 3, a["guide_path"], guide, dll=gpu_lib.dll, sink=sink)
    assert sink.tiles == 2                                                # no third call
    assert core_alignment_packed(K, a["member_path"], 3, a["guide_path"], guide, dll=gpu_lib.dll) == exp


def test_core_records_yields_nothing_when_a_row_fails(gpu_lib):
    """the reference's export returns Err and writes nothing: a letter the complement rejects in a block the guide reads in reverse"""
    import copy
    from pangraph_amd import batch
    from pangraph_amd.export import core_from_json, core_records
    g = copy.deepcopy(json.load(open(os.path.join(GOLDEN, "export_vectors.json")))["core_block_aln_general_case"]["graph"])
    args, keys, _ = core_from_json(g, "Path A")
    rows, core = er.expected_results(aligned=True, **args)
    rev = [c["block"] for c in core if c["reverse"]]
    assert rev and all(r["status"] == 0 for r in rows)
    bid = sorted(g["blocks"], key=int)[rev[0]]
    g["blocks"][bid]["consensus"] = g["blocks"][bid]["consensus"][:-1] + "x"
    assert any(r["status"] == 2 for r in er.expected_results(aligned=True, **core_from_json(g, "Path A")[0])[0])
    with pytest.raises(batch.PgaError, match="cannot be built"):
        core_records(g, "Path A", dll=gpu_lib.dll)
