"""Inputs for pga_join_graphs (pangraph_amd/join.py) and the expectation they are held against.  A case is a list of PARTS, each a dict graph
in the shape of simplify.normalize() ("g") and the tables of one part built from it ("t": join.Tables' input, with dead entries and with
insertion letters that are shared, shuffled and overlapping where the case says so).

`host_join` is the expectation: close.graph_tables(graph_join(...)) -- the dict union flattened in ascending block id, within a block in
ascending node id, paths in ascending path id -- plus origin and the two maps, which are read off the parts' tables by id.  `flat_join`
restates the header's text with loops over the tables, index after index; it stands in for the call where there is no device.
A case is {"parts": [{"g", "t"}], "exp": what JoinOut.to_lists() gives}."""
import copy
import functools

import numpy as np

import close_gen as cg
from pangraph_amd import close as cl
from pangraph_amd import join as jn
from pangraph_amd.assemble import _EditPool, _records
from pangraph_amd.close import TILE
from pangraph_amd.detach import DEL, INS, SUB

NONE = jn.NONE
EMPTY = {"blocks": {}, "paths": {}, "nodes": {}}


# ---------------------------------------------------------------- parts
def relabel(g, block=lambda b: b, path=lambda p: p, node=lambda n: n):
    """the graph with other ids"""
    return {"blocks": {block(b): {"consensus": v["consensus"], "alignments": {node(n): e for n, e in v["alignments"].items()}} for b, v in g["blocks"].items()},
            "paths": {path(p): dict(v, nodes=[node(n) for n in v["nodes"]]) for p, v in g["paths"].items()},
            "nodes": {node(n): dict(v, block_id=block(v["block_id"]), path_id=path(v["path_id"])) for n, v in g["nodes"].items()}}


def tables_of(g, rng=None, dead=()):
    """the tables of one part; rng: the insertion letters lie in a buffer with shared, shuffled and overlapping offsets behind 50 letters nobody names, otherwise dense"""
    blocks, paths, nodes, order = cg.graph_lists(g, {d: None for d in dead})
    edits = [g["blocks"][b[0]]["alignments"][n] for b in blocks for n in order[b[0]]]
    if rng is not None:
        pool = cg._Pool(rng)
        pool.buf += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 50))
        counts, subs, dels, inss = cg.flat_edits(edits, pool)
        letters = bytes(pool.buf)
    else:
        pool = _EditPool()
        counts = np.array([pool.add(e)[:3] for e in edits], np.uint32).reshape(-1, 3)
        subs, dels, inss, letters = _records(pool.subs, SUB), _records(pool.dels, DEL), _records(pool.inss, INS), bytes(pool.letters)
    return {"blocks": blocks, "paths": paths, "nodes": nodes, "rc_blocks": [(g["blocks"][b[0]]["consensus"].encode("latin-1"), b[2]) if b[3] else (b"", 0) for b in blocks],
            "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": letters, "who": [(n, int(g["nodes"][n]["strand"] == "-")) for b in blocks for n in order[b[0]]]}


def part(g, rng=None, dead=()):
    return {"g": g, "t": tables_of(g, rng, dead)}


def graph(seed, layout, k=0, stride=1, **kw):
    """a graph of close_gen.make_spec over `layout` ({block id: (cons_len, depth)}) whose path and node ids are x * stride + k: parts with different k never share one"""
    rng = np.random.default_rng(seed)
    spec = cg.make_spec(rng, layout, [], **kw)
    return relabel({f: spec[f] for f in ("blocks", "nodes", "paths")}, path=lambda p: p * stride + k, node=lambda n: n * stride + k)


# ---------------------------------------------------------------- the expectation: the dict route
def host_join(parts):
    g = copy.deepcopy(EMPTY)
    for p in parts:
        g = jn.graph_join(g, p["g"])
    t, order = cl.graph_tables(g)
    at = {b[0]: i for i, b in enumerate(t["blocks"])}
    path_at = {p[0]: i for i, p in enumerate(t["paths"])}
    member = {n: (k, m) for k, p in enumerate(parts) for m, (n, _) in enumerate(p["t"]["who"])}
    who = [(n, int(bool(r))) for n, r in t["who"]]
    subs, dels, inss = _records(t["subs"], SUB), _records(t["dels"], DEL), _records(t["inss"], INS)
    return {"blocks": [tuple(b) for b in t["blocks"]], "paths": [(p[0], p[1], p[2], int(bool(p[3]))) for p in t["paths"]],
            "nodes": [tuple(n[:5]) + (int(bool(n[5])),) for n in t["nodes"]], "rc_blocks": [(bytes(c), n) for c, n in t["rc_blocks"]],
            "counts": np.array(t["counts"], np.uint32).reshape(-1, 3), "subs": subs, "dels": dels, "inss": inss, "ins_seq": bytes(t["ins_seq"]), "who": who,
            "origin_part": [member[n][0] for n, _ in who], "origin": [member[n][1] for n, _ in who],
            "block_map": [at[b[0]] if b[3] else NONE for p in parts for b in p["t"]["blocks"]], "block_map_off": list(np.cumsum([0] + [len(p["t"]["blocks"]) for p in parts])),
            "path_map": [path_at[x[0]] for p in parts for x in p["t"]["paths"]], "path_map_off": list(np.cumsum([0] + [len(p["t"]["paths"]) for p in parts])),
            "totals": (len(t["blocks"]), len(t["paths"]), len(t["nodes"]), len(who), len(parts), len(subs), len(dels), len(inss), len(t["ins_seq"]))}


def build(parts):
    return {"parts": parts, "exp": host_join(parts)}


# ---------------------------------------------------------------- the call restated with loops over the tables
def flat_join(tables, flags=0):
    """pga_join_graphs on the tables of its parts restated with Python loops after the header's text -> what JoinOut.to_lists() gives"""
    def unique(ids, what):
        seen = set()
        for x in sorted(ids):
            if x in seen:
                raise jn.JoinError(f"Conflicting key: {what} id {x} is present twice")
            seen.add(x)
    alive = sorted((b[0], k, i) for k, t in enumerate(tables) for i, b in enumerate(t["blocks"]) if b[3])
    paths = sorted((p[0], k, i) for k, t in enumerate(tables) for i, p in enumerate(t["paths"]))
    unique([a[0] for a in alive], "block"); unique([p[0] for p in paths], "path"); unique([n[0] for t in tables for n in t["nodes"]], "node")
    first, off, src = [], [], []
    for t in tables:
        counts = np.asarray(t["counts"], np.int64).reshape(-1, 3)
        first.append(np.concatenate([[0], np.cumsum([b[2] if b[3] else 0 for b in t["blocks"]])]).astype(np.int64))
        o = np.zeros((len(counts) + 1, 3), np.int64)
        o[1:] = np.cumsum(counts, axis=0)
        off.append(o)
        src.append((counts, _records(t["subs"], SUB), _records(t["dels"], DEL), _records(t["inss"], INS), bytes(t["ins_seq"])))
    b_off = list(np.cumsum([0] + [len(t["blocks"]) for t in tables]))
    p_off = list(np.cumsum([0] + [len(t["paths"]) for t in tables]))
    block_map, path_map = [NONE] * b_off[-1], [NONE] * p_off[-1]
    o_blocks, rc, picked, who, o_part, origin = [], [], [], [], [], []
    for i, (bid, k, b) in enumerate(alive):
        t = tables[k]
        o_blocks.append((bid, t["blocks"][b][1], t["blocks"][b][2], 1)); rc.append((bytes(t["rc_blocks"][b][0]), t["blocks"][b][2]))
        block_map[b_off[k] + b] = i
        for s in range(t["blocks"][b][2]):
            m = int(first[k][b] + s)
            picked.append((k, m)); who.append((t["who"][m][0], int(bool(t["who"][m][1])))); o_part.append(k); origin.append(m)
    o_paths, o_nodes = [], []
    for i, (pid, k, p) in enumerate(paths):
        t = tables[k]
        _, node_off, n, circ = t["paths"][p]
        path_map[p_off[k] + p] = i
        o_paths.append((pid, len(o_nodes), n, int(bool(circ))))
        for nid, p0, p1, b, mem, rev in t["nodes"][node_off:node_off + n]:
            o_nodes.append((nid, p0, p1, block_map[b_off[k] + b], mem, int(bool(rev))))
    parts3 = [[src[k][1 + q][int(off[k][m, q]):int(off[k][m + 1, q])] for k, m in picked] for q in range(3)]
    cat = lambda q, dt: np.concatenate(parts3[q]) if parts3[q] else np.zeros(0, dt)
    subs, dels, inss = cat(0, SUB), cat(1, DEL), cat(2, INS).copy()
    seq, j = bytearray(), 0
    for (k, _), e in zip(picked, parts3[2]):
        for x in e:
            assert int(x["len"]) == 0 or int(x["seq_off"]) + int(x["len"]) <= len(src[k][4]), "seq_off + len of an insertion lies beyond its part's letter buffer"
            inss["seq_off"][j] = len(seq)
            seq += src[k][4][int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])]
            j += 1
    counts = np.array([src[k][0][m] for k, m in picked], np.uint32).reshape(-1, 3)
    return {"blocks": o_blocks, "paths": o_paths, "nodes": o_nodes, "rc_blocks": rc, "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": bytes(seq), "who": who,
            "origin_part": o_part, "origin": origin, "block_map": block_map, "block_map_off": b_off, "path_map": path_map, "path_map_off": p_off,
            "totals": (len(o_blocks), len(o_paths), len(o_nodes), len(picked), len(tables), len(subs), len(dels), len(inss), len(seq))}


# ---------------------------------------------------------------- the named cases
SMALL_LAYOUT = {50: (20, 3), 60: (30, 4), 70: (25, 5), 80: (10, 2), 90: (15, 0)}


def _two(layout0, layout1, seed, dead0=(), dead1=(), **kw):
    rng = np.random.default_rng(seed)
    return build([part(graph(seed, layout0, 0, 2, **kw), rng, dead0), part(graph(seed + 1, layout1, 1, 2, **kw), None, dead1)])


def _singleton(i, n, circular, reverse):
    seq = "".join("ACGT"[(i * 7 + j * j) % 4] for j in range(n))
    return {"g": jn.singleton_graph(i, seq, circular, reverse, f"s{i}"), "t": jn.singleton_tables(i, seq, circular, reverse)}


def _n_parts(n, seed):
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(n):
        layout = {int(b) * n + k: (int(rng.integers(1, 30)), int(rng.integers(0, 4))) for b in rng.integers(1, 1 << 40, int(rng.integers(1, 6)))}
        parts.append(part(graph(seed * 100 + k, layout, k, n, reverse=lambda b, j: (b + j) % 3 == 0, n_paths=1 + k % 3), rng if k % 2 == 0 else None, dead=[k] if k % 3 == 0 else ()))
    return build(parts)


def _with_empty_path(seed):
    rng = np.random.default_rng(seed)
    g0 = graph(seed, SMALL_LAYOUT, 0, 2, reverse=lambda b, k: k % 2 == 1)
    g1 = graph(seed + 1, {55: (12, 2), 95: (7, 1)}, 1, 2, reverse=lambda b, k: True)
    g1["paths"][3] = {"nodes": [], "circular": True, "tot_len": 0, "name": "empty"}
    g0["paths"][(1 << 64) - 2] = {"nodes": [], "circular": False, "tot_len": 0, "name": "empty too"}
    return build([part(g0, rng), part(g1)])


def _tile(n, before=0):
    return _two({5: (6, before), 9: (12, n), 11: (7, 3)}, {7: (9, 2), 10: (5, 3)}, 300 + n + before, edit_of=lambda rng, b, k, m: cg.random_edit(rng, m, (k % 3, k % 2, (k + 1) % 2)))


def _long_path(n):
    """one path of n nodes in one part (every node a member of one block), a short path in the other"""
    return _two({5: (6, n)}, {7: (9, 3)}, 400 + n, n_paths=1, edit_of=lambda rng, b, k, m: cg.edit())


def _letters():
    a = graph(16, {5: (30, 7), 9: (30, 8)}, 0, 2, edit_of=cg._letters)
    b = graph(17, {6: (30, 7), 8: (30, 5)}, 1, 2, edit_of=cg._letters)
    return build([part(a, np.random.default_rng(16)), part(b)])


def _buffer_end():
    """the last insertion of either part ends at its part's buffer end; the first part's buffer is longer than the second's"""
    a = graph(21, {5: (30, 2)}, 0, 2, edit_of=lambda rng, b, k, m: cg.edit([], [], [(3, "ACGTACGTAC" * (k + 1))]))
    b = graph(22, {6: (30, 1)}, 1, 2, edit_of=lambda rng, b, k, m: cg.edit([], [], [(0, "TTG")]))
    k = build([part(a), part(b)])
    for p in k["parts"]:
        last = p["t"]["inss"][-1]
        assert int(last["seq_off"]) + int(last["len"]) == len(p["t"]["ins_seq"])
    return k


def _high_index():
    half = lambda k: {2 * b + k: (3, 1 if b % 3500 == 0 else 0) for b in range(1, 35001)}
    return _two({**half(0), 80000: (12, 4)}, {**half(1), 80001: (9, 2)}, 10, edit_of=lambda rng, b, k, n: cg.random_edit(rng, n, (1, 0, 1)))


CASES = {
    "two_singletons": lambda: build([_singleton(5, 40, True, False), _singleton(3, 25, False, True)]),
    "alternating": lambda: _two({2 * b: (10 + b, b % 4) for b in range(1, 12)}, {2 * b + 1: (9 + b, (b + 1) % 4) for b in range(1, 12)}, 1),
    "left_below": lambda: _two({b: (10, 2) for b in range(1, 8)}, {b: (10, 2) for b in range(100, 105)}, 2),
    "left_above": lambda: _two({b: (10, 2) for b in range(100, 105)}, {b: (10, 2) for b in range(1, 8)}, 3),
    "id_extremes": lambda: _two({0: (8, 2), 1 << 63: (9, 1)}, {(1 << 64) - 1: (7, 2), 1: (5, 1)}, 4),
    "one_part_dead_entries": lambda: build([part(graph(5, SMALL_LAYOUT), np.random.default_rng(5), dead=(1, 2, 55, 65, 99))]),
    "empty_parts": lambda: build([part(copy.deepcopy(EMPTY)), part(graph(6, SMALL_LAYOUT, 0, 2), np.random.default_rng(6)), part(copy.deepcopy(EMPTY)),
                                  part(graph(7, {55: (12, 2), 95: (7, 1)}, 1, 2)), part(copy.deepcopy(EMPTY))]),
    "three_parts": lambda: _n_parts(3, 8),
    "eight_parts": lambda: _n_parts(8, 9),
    "singletons_1025": lambda: build([_singleton((i * 7919) % 4099, 1 + i % 9, i % 2 == 0, i % 3 == 0) for i in range(1025)]),
    "reverse_circular_empty_path": lambda: _with_empty_path(11),
    "two_nodes_of_one_path": lambda: _two({70: (25, 5)}, {71: (25, 4)}, 12, n_paths=1),
    "high_index": _high_index,
    "members_1023": lambda: _tile(TILE - 1),
    "members_1024": lambda: _tile(TILE),
    "members_1025": lambda: _tile(TILE + 1),
    "straddle": lambda: _tile(100, before=1000),
    "one_heavy": lambda: _two({5: (6, 3), 9: (40, 2001), 11: (7, 2)}, {10: (8, 2)}, 13, edit_of=cg._heavy),
    "list_lengths": lambda: _two({5: (200, 140)}, {9: (200, 140)}, 15, edit_of=cg._by_length),
    "letters": _letters,
    "buffer_end": _buffer_end,
    "second_level": lambda: _two({5: (30, 3)}, {9: (30, 3)}, 17, edit_of=cg._second_level),
    "path_1023": lambda: _long_path(TILE - 1),
    "path_1024": lambda: _long_path(TILE),
    "path_1025": lambda: _long_path(TILE + 1),
}
SMALL = ("two_singletons", "alternating", "left_below", "left_above", "id_extremes", "one_part_dead_entries", "empty_parts", "three_parts", "eight_parts", "reverse_circular_empty_path",
         "two_nodes_of_one_path", "letters", "buffer_end")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def shifted_close_graph(seed, k, n):
    """the graph before of close_gen.random_case(seed) with shifted ids: block ids (below 2^62 there) + k * 2^61, path and node ids x * n + k"""
    spec = cg.random_case(seed)["spec"]
    return relabel({f: spec[f] for f in ("blocks", "nodes", "paths")}, block=lambda b: b + (k << 61), path=lambda p: p * n + k, node=lambda x: x * n + k), [d + (k << 61) for d in spec["dead"]]


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """2 to 5 parts over the graphs of tests/close_gen.py with shifted ids"""
    rng = np.random.default_rng(900 + seed)
    n = int(rng.integers(2, 6))
    parts = []
    for k in range(n):
        g, dead = shifted_close_graph(int(rng.integers(0, 40)), k, n)
        parts.append(part(g, rng if rng.random() < 0.5 else None, dead))
    return build(parts)


def all_cases():
    return [(n, case(n)) for n in CASES] + [(f"random_{s}", random_case(s)) for s in range(40)]


# ---------------------------------------------------------------- comparisons
def same(got, want):
    """exact in every field -> the name of the first field that differs, or None (n_cons_letters, the tenth total, depends on the flag and is held elsewhere)"""
    if tuple(got["totals"][:9]) != tuple(want["totals"][:9]):
        return "totals"
    for f in ("blocks", "paths", "nodes", "rc_blocks", "who", "origin_part", "origin", "block_map", "block_map_off", "path_map", "path_map_off"):
        if [x for x in got[f]] != [x for x in want[f]]:
            return f
    if got["ins_seq"] != want["ins_seq"]:
        return "ins_seq"
    for f in ("counts", "subs", "dels", "inss"):
        if got[f].dtype != want[f].dtype or got[f].shape != want[f].shape or got[f].tobytes() != want[f].tobytes():
            return f
    return None


# ---------------------------------------------------------------- a case as a flat file for tests/emu/join_emu.cpp
def dump(k, path):
    """the parts in the C layouts, then the expectation: a u64 part count, then every array as a u64 byte count and its bytes, in the order join_emu.cpp's load()
    reads them (a block record with a pointer goes as the pair cons_len, n_members)"""
    import ctypes as C

    from pangraph_amd.topology import pack_lists
    raw = lambda arr, n: bytes(arr)[:n * C.sizeof(arr._type_)]
    pairs = lambda rows: np.array(rows, np.uint32).reshape(-1, 2).tobytes()
    blobs = []
    for p in k["parts"]:
        K = jn.Tables(p["t"])
        nb, B, n_paths, P, nn, N = K.graph
        blobs += [raw(B, nb), raw(P, n_paths), raw(N, nn), pairs([(len(c), n) for c, n in p["t"]["rc_blocks"]]), K.M.tobytes(), K.S.tobytes(), K.D.tobytes(), K.I.tobytes(), K.L, K.W.tobytes()]
    e = k["exp"]
    _, EB, _, EP, en, EN = pack_lists(e["blocks"], e["paths"], e["nodes"])
    blobs += [raw(EB, len(e["blocks"])), raw(EP, len(e["paths"])), raw(EN, en), e["counts"].tobytes(), e["subs"].tobytes(), e["dels"].tobytes(), e["inss"].tobytes(), e["ins_seq"],
              np.asarray(e["origin_part"], np.int32).tobytes(), np.asarray(e["origin"], np.int64).tobytes(), np.asarray(e["block_map"], np.uint32).tobytes(),
              np.asarray(e["path_map"], np.uint32).tobytes()]
    with open(path, "wb") as f:
        f.write(len(k["parts"]).to_bytes(8, "little"))
        for b in blobs:
            f.write(len(b).to_bytes(8, "little") + bytes(b))
