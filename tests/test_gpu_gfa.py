"""pga_export_gfa (pga_gfa.hip: `pangraph export gfa` built and formatted on the device) against the host restatement gfa.gfa_tables /
gfa.gfa_write_str on every named case of tests/gfa_gen.py, on seeded random graphs and on the plasmids: the joined sink bytes, the four
tables and n_bytes, verdict mode, tiles of 4 KB against the default; a sink that stops; the output of pga_plan_simplify by pointer; and
every malformed input but one: a file of 2^63 bytes needs 2^31 blocks or paths, its refusal is held by tests/emu/gfa_emu.cpp on the
host tables alone.  Every comparison is exact.  What each case holds is pinned by tests/test_gfa_cpu.py."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import gfa_gen as gg
import topo_gen as tg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import gfa  # noqa: E402
from pangraph_amd import topology as tp  # noqa: E402
from pangraph_amd.gfa import GfaParams  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "gfa_vectors.json")))
TABLES = ("segments", "links", "paths", "steps")


def call(args, cons, names, params, dll, sink=True):
    """-> (the joined bytes or None, the sizes of the pieces, {table: list}, n_bytes)"""
    pieces = []
    out = gfa.export_gfa_raw(args, cons, names, params, pieces.append if sink else None, steps=True, dll=dll)
    try:
        return (b"".join(pieces) if sink else None), [len(p) for p in pieces], {t: getattr(out, t)() for t in TABLES}, out.n_bytes
    finally:
        out.free()


def check(lists, cons, names, params, dll, monkeypatch, exp=None, default_tile=True):
    exp = exp or gfa.gfa_tables(*lists, params, cons, names)
    args, cons, names, alive = gg.pack(lists, cons, names)
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
    text, sizes, tables, n_bytes = call(args, cons, names, params, dll)
    assert text == exp["text"] and n_bytes == len(exp["text"])
    assert all(tables[t] == exp[t] for t in TABLES), [t for t in TABLES if tables[t] != exp[t]]
    assert sizes == [gg.EDGE] * (n_bytes // gg.EDGE) + ([n_bytes % gg.EDGE] if n_bytes % gg.EDGE else [])
    none, sizes, tables, n_bytes = call(args, cons, names, params, dll, sink=False)                            # verdict mode
    assert none is None and sizes == [] and n_bytes == len(exp["text"]) and all(tables[t] == exp[t] for t in TABLES)
    if default_tile:
        monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        text, sizes, _, _ = call(args, cons, names, params, dll)
        assert text == exp["text"] and len(sizes) == 1


# ---------------------------------------------------------------- 1. every named case, the random graphs, the graph past the second level
@pytest.mark.parametrize("name", sorted(gg.CASES))
def test_named_case(gpu_lib, monkeypatch, name):
    c = gg.case(name)
    check(c["lists"], c["cons"], c["names"], c["params"], gpu_lib.dll, monkeypatch, gg.expected(name))


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_graphs(gpu_lib, monkeypatch, seeds):
    for seed in seeds:
        c = gg.random_case(seed)
        for k, kw in enumerate(gg.PARAM_SETS):
            check(c["lists"], c["cons"], c["names"], GfaParams(**kw), gpu_lib.dll, monkeypatch, default_tile=(seed + k) % 4 == 0)


def test_past_the_second_level_of_the_tile_scan(gpu_lib, monkeypatch):
    arrays, exp = gg.second_level()
    args = gg.pack_arrays(arrays["blocks"], arrays["paths"], arrays["nodes"])
    for tile in ("4", None):
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", tile) if tile else monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        pieces = []
        out = gfa.export_gfa_raw(args, None, arrays["names"], arrays["params"], pieces.append, steps=True, dll=gpu_lib.dll)
        try:
            o = out.out
            assert (o.n_segments, o.n_links, o.n_paths, o.n_steps, o.n_bytes) == (len(exp["segments"]), len(exp["links"]), len(exp["paths"]), len(exp["steps"]), len(exp["text"]))
            assert b"".join(pieces) == exp["text"] and (tile is None or len(pieces) == (len(exp["text"]) + gg.EDGE - 1) // gg.EDGE)
            assert gg.view(o.steps, gg.NP_STEP, o.n_steps).tobytes() == np.array(exp["steps"], np.int64).astype(np.uint32).view(gg.NP_STEP).tobytes()
            assert out.segments() == exp["segments"] and out.links() == exp["links"] and out.paths() == exp["paths"]
        finally:
            out.free()


# ---------------------------------------------------------------- 2. the reference's vectors, the plasmids, files
@pytest.mark.parametrize("name", ["test_gfa_empty", "test_gfa_general_case"])
def test_reference_vectors(gpu_lib, monkeypatch, name):
    v = VEC[name]
    for tile in ("4", None):
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", tile) if tile else monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        assert gfa.export_gfa(v["graph"], GfaParams(**v["params"]), dll=gpu_lib.dll) == v["expected"].encode()


def test_plasmids(gpu_lib, monkeypatch, tmp_path):
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    for params in (None, GfaParams(include_sequences=True), GfaParams(minimum_depth=len(G["paths"]))):
        want = gfa.gfa_write_str(G, params)
        monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
        assert gfa.export_gfa(G, params, dll=gpu_lib.dll) == want
        monkeypatch.delenv("PGA_EXPORT_TILE_KB")
        assert gfa.export_gfa(G, params, dll=gpu_lib.dll) == want
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "8")
    assert gfa.write_gfa(G, str(tmp_path / "plasmids.gfa"), GfaParams(include_sequences=True), dll=gpu_lib.dll) == len(want := gfa.gfa_write_str(G, GfaParams(include_sequences=True)))
    assert (tmp_path / "plasmids.gfa").read_bytes() == want


# ---------------------------------------------------------------- 3. a sink that stops
@pytest.mark.parametrize("k", [1, 2, 3])
def test_sink_stops_at_call_k(gpu_lib, monkeypatch, k):
    c, exp = gg.case("long_p_line"), gg.expected("long_p_line")
    assert len(exp["text"]) > 3 * gg.EDGE
    args, cons, names, alive = gg.pack(c["lists"], c["cons"], c["names"])
    monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
    got = []
    with pytest.raises(batch.PgaError, match="^pga_export_gfa: sink stopped the export$"):
        gfa.export_gfa_raw(args, cons, names, c["params"], lambda piece: got.append(piece) or len(got) == k, dll=gpu_lib.dll)
    assert len(got) == k and b"".join(got) == exp["text"][:k * gg.EDGE]
    text, _, _, _ = call(args, cons, names, c["params"], gpu_lib.dll)                                          # the next call is whole
    assert text == exp["text"]


# ---------------------------------------------------------------- 4. the graph of pga_plan_simplify by pointer
@pytest.mark.parametrize("name", ["chain", "four_strands", "wrap_dropped_at_0", "high_indices"])
def test_plan_simplify_output_by_pointer(gpu_lib, monkeypatch, name):
    lists = tg.CASES[name]()
    host = tg.host_plan(*lists)
    assert host["round"]
    names = [b"path %d" % p[0] for p in lists[1]]
    plan = tp.plan_round_raw(tp.pack_lists(*lists), dll=gpu_lib.dll)
    try:
        args = plan.graph_args()
        for params in (GfaParams(), GfaParams(minimum_length=12), GfaParams(no_duplicated=True)):
            exp = gfa.gfa_tables(host["blocks"], host["paths"], host["nodes"], params, None, names)
            monkeypatch.setenv("PGA_EXPORT_TILE_KB", "4")
            text, _, tables, n_bytes = call(args, None, names, params, gpu_lib.dll)
            assert text == exp["text"] and n_bytes == len(text) and all(tables[t] == exp[t] for t in TABLES)
    finally:
        plan.free()


# ---------------------------------------------------------------- 5. malformed input: -1, a message, a zeroed output
def raw(dll, lists, cons, names, prm, flags=0, sink=None, name_len=None):
    gfa._bind(dll)
    args, _, _, alive = gg.pack(lists, None, None)
    cons_p, _, keep_c = gfa._bytes_array(cons, len(lists[0]))
    names_p, names_l, keep_n = gfa._bytes_array(names, len(lists[1]))
    if name_len is not None:
        names_l = (C.c_uint32 * len(name_len))(*name_len)
    out = gfa.gfa_out_t()
    C.memset(C.addressof(out), 0xAB, C.sizeof(out))
    p = prm.to_c() if prm is not None else None
    rc = dll.pga_export_gfa(*args, gfa._ptr(cons_p), gfa._ptr(names_p), gfa._ptr(names_l), C.cast(C.byref(p), C.c_void_p) if p is not None else None, flags, C.byref(out),
                            C.cast(sink, C.c_void_p) if sink is not None else None, None)
    image, err = bytes(out), dll.pga_last_error().decode() if rc != 0 else ""
    if rc == 0:
        dll.pga_gfa_free(C.byref(out))
    return rc, image, err


def _base():
    c = gg.case("no_duplicated_off")                                        # blocks A D E; paths "D+ A+ D- E+" and circular "E- A+"
    return [list(x) for x in c["lists"]], list(c["cons"]), list(c["names"])


def _node(n, **kw):
    f = dict(zip(("node_id", "pos0", "pos1", "block", "member", "reverse"), n), **kw)
    return tuple(f[k] for k in ("node_id", "pos0", "pos1", "block", "member", "reverse"))


MALFORMED = {
    "member_out_of_range": (lambda L, c, n: L[2].__setitem__(0, _node(L[2][0], member=2)), "member >= depth"),
    "block_out_of_range": (lambda L, c, n: L[2].__setitem__(0, _node(L[2][0], block=3)), "block out of range"),
    "dead_block": (lambda L, c, n: (L[0].insert(3, (9, 5, 0, 0)), L[2].__setitem__(1, _node(L[2][1], block=3))), "dead block"),
    "node_off": (lambda L, c, n: L[1].__setitem__(1, (2, 5, 2, 1)), "node_off is not the running sum"),
    "n_nodes_sum": (lambda L, c, n: L[1].__setitem__(1, (2, 4, 1, 1)), "do not sum to the node count"),
    "path_ids": (lambda L, c, n: L[1].__setitem__(1, (1, 4, 2, 1)), "path ids are not ascending"),
    "block_ids": (lambda L, c, n: L[0].__setitem__(2, (2, 10, 2, 1)), "not strictly ascending"),
    "slot_twice": (lambda L, c, n: L[2].__setitem__(2, _node(L[2][2], member=0)), "slot is named by"),
    "depth_sum": (lambda L, c, n: L[0].__setitem__(0, (1, 10, 3, 1)), "do not sum to its depth"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_malformed_graph(gpu_lib, name):
    L, cons, names = _base()
    assert raw(gpu_lib.dll, L, cons, names, GfaParams())[0] == 0
    change, message = MALFORMED[name]
    change(L, cons, names)
    rc, out, err = raw(gpu_lib.dll, L, cons + [b""] * (len(L[0]) - len(cons)), names, GfaParams(include_sequences=True))
    assert rc == -1 and out == bytes(len(out)) and err.startswith("pga_export_gfa: ") and message in err, err


def test_malformed_parameters_letters_and_names(gpu_lib):
    L, cons, names = _base()
    dll, seq = gpu_lib.dll, GfaParams(include_sequences=True)
    bad = lambda r, message: r[0] == -1 and r[1] == bytes(len(r[1])) and r[2].startswith("pga_export_gfa: ") and message in r[2]
    assert bad(raw(dll, L, cons, names, None), "null parameters")
    assert bad(raw(dll, L, cons, names, GfaParams(minimum_length=5, maximum_length=4)), "minimum_length above maximum_length")
    assert bad(raw(dll, L, cons, names, GfaParams(minimum_depth=3, maximum_depth=2)), "minimum_depth above maximum_depth")
    assert bad(raw(dll, L, cons, names, GfaParams(), flags=2), "unknown flag")
    assert bad(raw(dll, L, None, names, seq), "without consensus letters")
    assert bad(raw(dll, L, [cons[0], None, cons[2]], names, seq), "null consensus of an emitted block (block 1)")
    assert bad(raw(dll, L, cons, None, GfaParams()), "null names")
    assert bad(raw(dll, L, cons, [names[0], None], GfaParams(), name_len=[2, 2]), "null name of an emitted path (path 1)")
    # what is not emitted is not read: the duplicated block's NULL consensus with no_duplicated, a NULL name of zero length
    assert raw(dll, L, [cons[0], None, cons[2]], names, GfaParams(include_sequences=True, no_duplicated=True))[0] == 0
    assert raw(dll, L, None, [names[0], None], GfaParams())[0] == 0
    assert raw(dll, L, None, None, GfaParams(minimum_length=11))[0] == 0                                        # everything filtered: no name is needed


def test_no_paths_or_no_nodes_is_the_header_line(gpu_lib):
    got = []
    out = gfa.export_gfa_raw(gg.pack(([(1, 5, 0, 1)], [], []), None, [])[0], None, [], None, got.append, steps=True, dll=gpu_lib.dll)
    assert got == [gfa.HEADER] and out.n_bytes == len(gfa.HEADER) and (out.segments(), out.links(), out.paths(), out.n_steps) == ([], [], [], 0)
    out.free()
    got = []
    out = gfa.export_gfa_raw(gg.pack(([(1, 5, 0, 1)], [(1, 0, 0, 1), (2, 0, 0, 0)], []), None, [b"a", b"b"])[0], None, [b"a", b"b"], None, got.append, dll=gpu_lib.dll)
    assert got == [gfa.HEADER] and out.n_bytes == len(gfa.HEADER) and out.steps() is None
    out.free()
