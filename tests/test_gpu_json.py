"""pga_export_json (pga_json.hip: the pangraph JSON built and formatted on the device) against the host restatement jsonout.json_tables /
json_write_str on every named case of tests/json_gen.py, on seeded random graphs, on the graph past the second level of the tile scan and
on the plasmids, whose file is the reference's own: the joined sink bytes, n_bytes, the offsets and node_order, verdict mode, tiles of 4 KB
against the default; a sink that stops; the output of pga_remove_paths by pointer; and every malformed input but one: a file of 2^63
bytes cannot be made here, its refusal is held by tests/emu/json_emu.cpp on the host tables alone.  Every comparison is exact.  What
each case holds is pinned by tests/test_json_cpu.py."""
import copy
import ctypes as C
import gzip
import hashlib
import json
import os

import pytest

import json_gen as jg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import jsonout  # noqa: E402
from pangraph_amd import remove as rm  # noqa: E402
from pangraph_amd import simplify as sp  # noqa: E402
from pangraph_amd.reconsensus import rc_member_t  # noqa: E402

PLASMIDS = os.path.join(GOLDEN, "plasmids.json.gz")
TABLES = ("section_off", "path_off", "block_off", "node_order")


def call(F, dll, sink=True):
    """F: anything with graph_args, block_args, path_meta, ins_seq_len -> (the joined bytes or None, the sizes of the pieces, {table: list}, n_bytes)"""
    pieces = []
    out = jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, pieces.append if sink else None, F.ins_seq_len, dll=dll)
    try:
        return (b"".join(pieces) if sink else None), [len(p) for p in pieces], {"section_off": out.section_off, "path_off": out.path_off(), "block_off": out.block_off(), "node_order": out.node_order()}, out.n_bytes
    finally:
        out.free()


def check(F, exp, dll, monkeypatch, default_tile=True):
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
    text, sizes, tables, n_bytes = call(F, dll)
    assert text == exp["text"] and n_bytes == len(exp["text"])
    assert all(tables[t] == exp[t] for t in TABLES), [t for t in TABLES if tables[t] != exp[t]]
    assert sizes == [jg.EDGE] * (n_bytes // jg.EDGE) + ([n_bytes % jg.EDGE] if n_bytes % jg.EDGE else [])
    none, sizes, tables, n_bytes = call(F, dll, sink=False)                  # verdict mode
    assert none is None and sizes == [] and n_bytes == len(exp["text"]) and all(tables[t] == exp[t] for t in TABLES)
    if default_tile:
        monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        text, sizes, _, _ = call(F, dll)
        assert text == exp["text"] and len(sizes) == 1


# ---------------------------------------------------------------- 1. every named case, the random graphs, the graph past the second level
@pytest.mark.parametrize("name", sorted(jg.CASES))
def test_named_case(gpu_lib, monkeypatch, name):
    check(jg.flat(jg.case(name)), jg.expected(name), gpu_lib.dll, monkeypatch)


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_graphs(gpu_lib, monkeypatch, seeds):
    for seed in seeds:
        c = jg.random_case(seed)
        check(jg.flat(c), jg.expected_of(c), gpu_lib.dll, monkeypatch, default_tile=seed % 4 == 0)


def test_past_the_second_level_of_the_tile_scan(gpu_lib, monkeypatch):
    args, block_args, meta, _, sha, n_bytes, sec = jg.big()
    for tile in ("1024", None):
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", tile) if tile else monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        h, sizes = hashlib.sha256(), []
        out = jsonout.export_json_raw(args, block_args, meta, lambda piece: (h.update(piece), sizes.append(len(piece))) and None, 0, dll=gpu_lib.dll)
        try:
            assert out.n_bytes == n_bytes == sum(sizes) and h.hexdigest() == sha and max(sizes) <= (int(tile) << 10 if tile else 16 << 20) and len(sizes) == -(-n_bytes // max(sizes))
            assert out.path_off() == [19] and out.block_off() == [sec[1] + 16] and out.node_order() == [0] and out.section_off == sec
        finally:
            out.free()


# ---------------------------------------------------------------- 2. the reference's own file
def test_plasmids(gpu_lib, monkeypatch, tmp_path):
    want = gzip.open(PLASMIDS, "rb").read()
    G = json.loads(want)
    for tile in ("4", "64", None):
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", tile) if tile else monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        assert jsonout.export_json(G, dll=gpu_lib.dll) == want
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "8")
    assert jsonout.write_json(PLASMIDS, str(tmp_path / "plasmids.json"), dll=gpu_lib.dll) == len(want) and (tmp_path / "plasmids.json").read_bytes() == want
    exp, F = jsonout.json_tables(G), jsonout.json_from_json(G)
    _, _, tables, _ = call(F, gpu_lib.dll, sink=False)
    assert all(tables[t] == exp[t] for t in TABLES)


# ---------------------------------------------------------------- 3. a sink that stops
@pytest.mark.parametrize("k", [1, 2, 3])
def test_sink_stops_at_call_k(gpu_lib, monkeypatch, k):
    F, exp = jg.flat(jg.case("long_name_desc")), jg.expected("long_name_desc")
    assert len(exp["text"]) > 4 * jg.EDGE
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
    got = []
    with pytest.raises(batch.PgaError, match="^pga_export_json: sink stopped the export$"):
        jsonout.export_json_raw(F.graph_args, F.block_args, F.path_meta, lambda piece: got.append(piece) or len(got) == k, F.ins_seq_len, dll=gpu_lib.dll)
    assert len(got) == k and b"".join(got) == exp["text"][:k * jg.EDGE]
    assert call(F, gpu_lib.dll)[0] == exp["text"]                            # the next call is whole


# ---------------------------------------------------------------- 4. the output of pga_remove_paths by pointer
def as_json(g):
    """a graph of simplify.normalize -> the pangraph JSON the restatement takes (normalize keeps no description: null)"""
    edit = lambda e: {"subs": [{"pos": p, "alt": a} for p, a in e["subs"]], "dels": [{"pos": p, "len": n} for p, n in e["dels"]], "inss": [{"pos": p, "seq": s} for p, s in e["inss"]]}
    return {"paths": {str(k): dict(p, desc=None) for k, p in g["paths"].items()}, "nodes": {str(k): dict(n, position=list(n["position"])) for k, n in g["nodes"].items()},
            "blocks": {str(k): {"consensus": b["consensus"], "alignments": {str(n): edit(e) for n, e in b["alignments"].items()}} for k, b in g["blocks"].items()}}


@pytest.mark.parametrize("n_paths,flags", [(1, 0), (3, rm.COMPACT_LETTERS), (8, 0)])
def test_remove_paths_output_by_pointer(gpu_lib, monkeypatch, n_paths, flags):
    G = json.load(gzip.open(PLASMIDS))
    g = sp.normalize(G)
    focal = set(G["paths"][k]["name"] for k in sorted(G["paths"], key=int)[:n_paths])
    want = copy.deepcopy(g)
    for pid in [pid for pid in sorted(want["paths"]) if want["paths"][pid]["name"] not in focal]:
        sp.remove_path(want, pid)
    exp = jsonout.json_tables(as_json(want))
    R = rm.removed_graph(g, focal, "device", gpu_lib.dll, flags)
    try:
        out = R.out
        assert R.g == want and out.out.n_dead_blocks > 0
        alive = iter(exp["block_off"])
        exp["block_off"] = [next(alive) if out.out.blocks[b].alive else jg.U64 for b in range(out.out.n_blocks)]

        class View:
            graph_args, block_args = out.graph_args(), out.block_args()
            path_meta = [(want["paths"][pid]["tot_len"], want["paths"][pid]["name"].encode(), None) for pid in sorted(want["paths"])]
            ins_seq_len = out.out.n_ins_letters if flags else C.sizeof(out.keep_alive[0].L)
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", "64")
        text, _, tables, n_bytes = call(View, gpu_lib.dll)
        assert text == exp["text"] and n_bytes == len(text) and all(tables[t] == exp[t] for t in TABLES)
    finally:
        R.close()


# ---------------------------------------------------------------- 5. malformed input: -1, a message, a zeroed output
def _base():
    """two paths over three blocks (one dead entry between them), every kind of edit -> a Flat whose arrays the tests change in place"""
    e1 = {"subs": [(1, "T"), (2, "G")], "dels": [(3, 1)], "inss": [(0, "ACGT"), (4, "G")]}
    return jg.flat(jg.build([(1, "ACGTA"), None, (5, "GG"), (9, "TTT")], [(1, False, 9, "p", "d", [jg.node(21, 0, e1), jg.node(22, 2), jg.node(23, 0)]), (2, True, 3, "q", None, [jg.node(24, 3, e1), jg.node(25, 0)])]))


def raw(dll, F, flags=0, sink=None, **override):
    """the call with the arguments of jsonout.marshal, some of them replaced by name -> (rc, the bytes of out, the message)"""
    jsonout._bind(dll)
    args, keep = jsonout.marshal(F.graph_args, F.block_args, F.path_meta, F.ins_seq_len)
    names = ["n_blocks", "blocks", "n_paths", "paths", "n_nodes", "nodes", "cons", "members", "subs", "dels", "inss", "ins_seq", "ins_seq_len", "tot_len", "names", "name_len", "descs", "desc_len"]
    for k, v in override.items():
        args[names.index(k)] = v
    out = jsonout.json_out_t()
    C.memset(C.addressof(out), 0xAB, C.sizeof(out))
    rc = dll.pga_export_json(*args, flags, C.byref(out), C.cast(sink, C.c_void_p) if sink is not None else None, None)
    image, err = bytes(out), dll.pga_last_error().decode() if rc != 0 else ""
    if rc == 0:
        dll.pga_json_free(C.byref(out))
    return rc, image, err


def bad(r, message):
    return r[0] == -1 and r[1] == bytes(len(r[1])) and r[2].startswith("pga_export_json: ") and message in r[2]


def _node(F, i, **kw):
    for k, v in kw.items():
        setattr(F.graph_args[5][i], k, v)


def _deeper(F):
    """block 2 claims a second member that no node names; the member list grows by its (empty) entry, as the contract asks"""
    F.graph_args[1][2].depth = 2
    old = [(m.n_subs, m.n_dels, m.n_inss) for m in F.M]
    F.M = (rc_member_t * 6)(*[rc_member_t(*x) for x in old[:4] + [(0, 0, 0)] + old[4:]])
    F.block_args = F.block_args[:2] + (F.M,) + F.block_args[3:]


MALFORMED_GRAPH = {
    "member_out_of_range": (lambda F: _node(F, 0, member=3), "member >= depth"),
    "block_out_of_range": (lambda F: _node(F, 0, block=4), "block out of range"),
    "dead_block": (lambda F: _node(F, 1, block=1), "dead block"),
    "node_off": (lambda F: setattr(F.graph_args[3][1], "node_off", 4), "node_off is not the running sum"),
    "n_nodes_sum": (lambda F: setattr(F.graph_args[3][1], "n_nodes", 1), "do not sum to the node count"),
    "path_ids": (lambda F: setattr(F.graph_args[3][1], "path_id", 1), "path ids are not ascending"),
    "block_ids": (lambda F: setattr(F.graph_args[1][2], "block_id", 1), "not strictly ascending"),
    "slot_twice": (lambda F: _node(F, 2, member=0), "slot is named by"),
    "depth_sum": (_deeper, "do not sum to its depth"),
    "node_id_twice_in_a_block": (lambda F: _node(F, 2, node_id=21), "two nodes with one node_id"),
    "node_id_twice_across_blocks": (lambda F: _node(F, 3, node_id=22), "two nodes with one node_id"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED_GRAPH))
def test_malformed_graph(gpu_lib, name):
    F = _base()
    assert raw(gpu_lib.dll, F)[0] == 0
    change, message = MALFORMED_GRAPH[name]
    change(F)
    assert bad(r := raw(gpu_lib.dll, F), message), r[2]
    assert raw(gpu_lib.dll, _base())[0] == 0                                 # the library goes on


def test_malformed_arguments(gpu_lib):
    dll, F = gpu_lib.dll, _base()
    assert bad(raw(dll, F, flags=1), "unknown flag")
    assert bad(raw(dll, F, members=None), "null members")
    for k in ("subs", "dels", "inss"):
        assert bad(raw(dll, F, **{k: None}), "null edit list with a non-zero count")
    assert bad(raw(dll, F, ins_seq=None), "null insertion letters")
    for k in ("tot_len", "names", "name_len", "descs", "desc_len"):
        assert bad(raw(dll, F, **{k: None}), "null tot_len, names or descs")
    assert bad(raw(dll, F, cons=None), "null consensus of an alive block (block 0)")
    args, keep = jsonout.marshal(F.graph_args, F.block_args, F.path_meta, F.ins_seq_len)
    cons = (C.c_void_p * 4)(*[keep[4][b] for b in range(4)])
    cons[2] = None
    assert bad(raw(dll, F, cons=C.cast(cons, C.c_void_p)), "null consensus of an alive block (block 2)")
    cons[2], cons[1] = keep[4][2], None                                      # a dead entry's pointer is not read
    assert raw(dll, F, cons=C.cast(cons, C.c_void_p))[0] == 0
    E = jg.flat(jg.build([(1, ""), (2, "")], [(1, False, 0, None, None, [jg.node(5, 1)])]))
    assert raw(dll, E, cons=None, ins_seq=None, subs=None, dels=None, inss=None)[0] == 0       # nothing to read: empty consensus, no edit
    assert raw(dll, F)[0] == 0


@pytest.mark.parametrize("alt", [0x1f, 0x7f, ord('"'), ord("\\"), 0x80, 0x141, 0])
def test_substitution_letter_json_would_escape(gpu_lib, alt):
    F = _base()
    F.S[3].alt = alt
    assert bad(r := raw(gpu_lib.dll, F), "a substitution letter that JSON would escape (sub 3)"), r[2]


def test_insertion_letters_and_ranges(gpu_lib):
    dll = gpu_lib.dll
    for letter in (b"\n", b'"', b"\\", b"\x7f", b"\x1f", b"\xc3"):
        F = _base()
        C.memmove(C.addressof(F.L) + 7, letter, 1)                              # the third letter of insertion 2 ("ACGT" of the second member with edits)
        assert bad(r := raw(dll, F), "an insertion letter that JSON would escape (insertion 2)"), r[2]
    F = _base()
    assert F.ins_seq_len == 10 and (F.I[3].seq_off, F.I[3].len) == (9, 1)
    assert bad(raw(dll, F, ins_seq_len=9), "runs past the insertion letters (insertion 3)")
    F.I[1].seq_off = 10
    assert bad(raw(dll, F), "runs past the insertion letters (insertion 1)")
    F.I[1].seq_off, F.I[1].len = 9, 0xffffffff
    assert bad(raw(dll, F), "runs past the insertion letters (insertion 1)")
    F.I[1].seq_off, F.I[1].len = (1 << 64) - 1, 1
    assert bad(raw(dll, F), "runs past the insertion letters (insertion 1)")
    F.I[1].seq_off, F.I[1].len = 10, 0                                       # an empty insertion at the very end is in range
    assert raw(dll, F)[0] == 0


def test_empty_graph_is_three_empty_maps(gpu_lib):
    E = jg.flat(jg.build([], []))
    got = []
    out = jsonout.export_json_raw(E.graph_args, E.block_args, E.path_meta, got.append, 0, dll=gpu_lib.dll)
    assert got == [jsonout.EMPTY] and out.n_bytes == 48 and out.section_off == [4, 19, 35] and (out.path_off(), out.block_off(), out.node_order()) == ([], [], [])
    out.free()
    with pytest.raises(batch.PgaError, match="sink stopped the export"):
        jsonout.export_json_raw(E.graph_args, E.block_args, E.path_meta, lambda piece: True, 0, dll=gpu_lib.dll)
    assert jsonout.export_json({"paths": {}, "blocks": {}, "nodes": {}}, dll=gpu_lib.dll) == jsonout.EMPTY
