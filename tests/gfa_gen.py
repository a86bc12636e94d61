"""Graphs for pga_export_gfa (pangraph_amd/gfa.py, pga_gfa.hip): every named case is the smallest graph with its property and carries a
pin -- what tests/test_gfa_cpu.py holds against the host restatement (gfa.gfa_tables) before tests/test_gpu_gfa.py relies on it -- and,
where it is small, the text written out by hand.  A case is {"lists": (blocks, paths, nodes) as topology.pack_lists takes them, "cons":
per block bytes, "names": per path bytes, "params": GfaParams, "pin": exp -> truth, "text": bytes or None, "json": whether to_json() can
hold it}.  The tile cases are made for PGA_EXPORT_TILE_KB=4: EDGE is the first tile edge."""
import ctypes as C
import functools
import random

import numpy as np

from pangraph_amd import gfa
from pangraph_amd.gfa import GfaParams

EDGE = 4096                              # PGA_EXPORT_TILE_KB=4
TILE = 1024                              # PGA_TOPO_TILE
SCAN_THREADS = 256
EDIT = {"subs": [], "dels": [], "inss": []}
LETTERS = "ACGT"
NP_BLOCK = np.dtype([("block_id", "<u8"), ("cons_len", "<u4"), ("depth", "<u4"), ("alive", "<i4"), ("pad", "<i4")])
NP_PATH = np.dtype([("path_id", "<u8"), ("node_off", "<u8"), ("n_nodes", "<u4"), ("circular", "<i4")])
NP_NODE = np.dtype([("node_id", "<u8"), ("pos0", "<u8"), ("pos1", "<u8"), ("block", "<u4"), ("member", "<u4"), ("reverse", "<i4"), ("pad", "<i4")])
NP_SEGMENT = np.dtype([("block", "<u4"), ("depth", "<u4"), ("cons_len", "<u4"), ("duplicated", "<i4"), ("byte_off", "<u8")])
NP_EDGE = np.dtype([("b1", "<u4"), ("b2", "<u4"), ("s1", "<i4"), ("s2", "<i4"), ("count", "<u4"), ("pad", "<u4")])
NP_GPATH = np.dtype([("path", "<u4"), ("n_steps", "<u4"), ("step_off", "<u8"), ("byte_off", "<u8")])
NP_STEP = np.dtype([("block", "<u4"), ("reverse", "<i4")])


def letters(bid, n):
    """the consensus of a block: a pattern that depends on its id, so that a copy from the wrong block or offset shows"""
    return bytes(ord(LETTERS[(bid * 7 + k * k + k // 3) % 4]) for k in range(n)) if n < 4096 else (letters(bid, 1024) * (n // 1024 + 1))[:n]


def graph(paths, lens=None, ids=None, names=None, cons=True):
    """paths: [(circular, "A+ B- ...")], blocks named by a word; lens / ids: {word: cons_len / block id} (default 10, 1 + rank by name);
    names: per path str / bytes (default "p<k>").  Node ids are 101, 102, ... in path order and the members of a block are ordered by node
    id -> (lists, cons, names)"""
    words = sorted({w[:-1] for _, s in paths for w in s.split()} | set(lens or {}) | set(ids or {}))
    bid = {w: (ids or {}).get(w, 1 + r) for r, w in enumerate(words)}
    words.sort(key=lambda w: bid[w])
    at = {w: i for i, w in enumerate(words)}
    depth = {w: 0 for w in words}
    p_list, n_list, nid = [], [], 100
    for k, (circular, s) in enumerate(paths):
        p_list.append((k + 1, len(n_list), len(s.split()), 1 if circular else 0))
        for w in s.split():
            nid += 1
            n_list.append((nid, 0, 0, at[w[:-1]], depth[w[:-1]], w[-1] == "-"))
            depth[w[:-1]] += 1
    b_list = [(bid[w], (lens or {}).get(w, 10), depth[w], 1) for w in words]
    enc = lambda x: x.encode() if isinstance(x, str) else x
    return ((b_list, p_list, n_list), [letters(b[0], b[1]) for b in b_list] if cons else None, [enc(x) for x in (names or [f"p{k + 1}" for k in range(len(paths))])])


def shift_blocks(lists, cons, by):
    """the same graph behind `by` dead block entries: every block index grows by `by`"""
    blocks, paths, nodes = lists
    return ([(0, 0, 0, 0)] * by + blocks, paths, [(n[0], n[1], n[2], n[3] + by, n[4], n[5]) for n in nodes]), ([None] * by + cons) if cons else None


def to_json(case):
    """the pangraph JSON of a case (alive blocks only): what gfa.gfa_write_str and gfa.gfa_from_json take"""
    (blocks, paths, nodes), cons, names = case["lists"], case["cons"], case["names"]
    g = {"paths": {}, "nodes": {}, "blocks": {str(b[0]): {"id": b[0], "consensus": cons[i].decode(), "alignments": {}} for i, b in enumerate(blocks) if b[3]}}
    for k, (pid, off, n, circular) in enumerate(paths):
        g["paths"][str(pid)] = {"id": pid, "nodes": [x[0] for x in nodes[off:off + n]], "tot_len": 0, "circular": bool(circular), "name": names[k].decode()}
        for nid, pos0, pos1, b, _, rev in nodes[off:off + n]:
            g["nodes"][str(nid)] = {"id": nid, "block_id": blocks[b][0], "path_id": pid, "strand": "-" if rev else "+", "position": [pos0, pos1]}
            g["blocks"][str(blocks[b][0])]["alignments"][str(nid)] = EDIT
    return g


def _case(made, params=None, pin=None, text=None, json=True):
    lists, cons, names = made
    return {"lists": lists, "cons": cons, "names": names, "params": params or GfaParams(), "pin": pin or (lambda e: True), "text": text, "json": json}


def line_at(exp, prefix):
    """the byte offset of the first line of the text that starts with `prefix`"""
    t = exp["text"]
    return 0 if t.startswith(prefix) else t.index(b"\n" + prefix) + 1


# ---------------------------------------------------------------- ids, widths and names
def _width_ids():
    ids = {"A": 9, "B": 10, "C": 99, "D": 100, "E": 10 ** 19 - 1, "F": 10 ** 19, "G": 2 ** 64 - 1}
    return _case(graph([(False, "A+ B- C+ D- E+ F- G+"), (True, "G- A+")], ids=ids, lens={"A": 9, "B": 10, "C": 99, "D": 100, "E": 1, "F": 1, "G": 3}),
                 pin=lambda e: b"\t18446744073709551615-,9+\t" in e["text"] and b"L\t9999999999999999999\t+\t10000000000000000000\t-\t" in e["text"]
                 and b"S\t99\t*\tRC:i:99\tLN:i:99\n" in e["text"] and b"S\t100\t*\tRC:i:100\tLN:i:100\n" in e["text"] and b"RC:i:6\tLN:i:3" in e["text"])


def _width_counts():
    """links and depths of 9, 10, 99 and 100: so many two-node paths each"""
    paths = [(False, f"{a}+ {b}+") for a, b, n in (("A", "B", 9), ("C", "D", 10), ("E", "F", 99), ("G", "H", 100)) for _ in range(n)]
    want = [b"L\t1\t+\t2\t+\t*\tRC:i:9\n", b"L\t3\t+\t4\t+\t*\tRC:i:10\n", b"L\t5\t+\t6\t+\t*\tRC:i:99\n", b"L\t7\t+\t8\t+\t*\tRC:i:100\n",
            b"S\t1\t*\tRC:i:90\tLN:i:10\n", b"S\t8\t*\tRC:i:1000\tLN:i:10\n"]
    return _case(graph(paths), pin=lambda e: all(w in e["text"] for w in want) and len(e["links"]) == 4 and len(e["paths"]) == 218)


def _rc_above_2_32():
    lists, _, names = graph([(False, "A+ B+"), (False, "A-"), (True, "A+")], lens={"A": 2 ** 31 + 5, "B": 2 ** 32 - 1}, cons=False)
    return _case((lists, None, names), pin=lambda e: b"S\t1\t*\tRC:i:6442450959\tLN:i:2147483653\n" in e["text"] and b"RC:i:4294967295\tLN:i:4294967295\n" in e["text"], json=False)


def _names():
    names = ["", "two words\tand a tab", "plásmido 中文 \U0001f9ec"]
    return _case(graph([(False, "A+"), (True, "B-"), (False, "A- B+")], names=names),
                 pin=lambda e: b"\nP\t\t1+\t*\n" in e["text"] and "plásmido 中文 \U0001f9ec".encode() in e["text"],
                 text=b"H\tVN:Z:1.0\n# blocks\nS\t1\t*\tRC:i:20\tLN:i:10\nS\t2\t*\tRC:i:20\tLN:i:10\n# edges\nL\t1\t-\t2\t+\t*\tRC:i:1\nL\t2\t+\t2\t+\t*\tRC:i:1\n# paths\n"
                      b"P\t\t1+\t*\nP\ttwo words\tand a tab\t2-\t*\tTP:Z:circular\nP\t" + "plásmido 中文 \U0001f9ec".encode() + b"\t1-,2+\t*\n")


# ---------------------------------------------------------------- filtering
def _bounds_graph():
    """lengths 9, 10, 11 with depth 2 (L9 L10 L11), depths 1, 2, 3 with length 20 (D1 D2 D3); ids in that order"""
    return graph([(False, "L09+ L10+ L11+ D1+ D2+ D3+"), (False, "L09- L10- L11- D2- D3-"), (False, "D3+")], lens={"L09": 9, "L10": 10, "L11": 11, "D1": 20, "D2": 20, "D3": 20},
                 ids={"L09": 1, "L10": 2, "L11": 3, "D1": 4, "D2": 5, "D3": 6})


BOUNDS = {   # name: (params, the ids of the segments left)
    "min_len_at": (dict(minimum_length=10), [2, 3, 4, 5, 6]), "min_len_off": (dict(minimum_length=11), [3, 4, 5, 6]),
    "max_len_at": (dict(maximum_length=10), [1, 2]), "max_len_off": (dict(maximum_length=9), [1]),
    "min_depth_at": (dict(minimum_depth=2), [1, 2, 3, 5, 6]), "min_depth_off": (dict(minimum_depth=3), [6]),
    "max_depth_at": (dict(maximum_depth=2), [1, 2, 3, 4, 5]), "max_depth_off": (dict(maximum_depth=1), [4]),
}


def _bounds(which):
    params, left = BOUNDS[which]
    return _case(_bounds_graph(), GfaParams(**params), pin=lambda e: [s[0] + 1 for s in e["segments"]] == left)


def _no_duplicated(on):
    # D has two non-adjacent nodes on path 1; E has depth 2 on two different paths and is not duplicated
    made = graph([(False, "D+ A+ D- E+"), (True, "E- A+")])
    if on:
        return _case(made, GfaParams(no_duplicated=True), pin=lambda e: [s[0] for s in e["segments"]] == [0, 2] and (0, 2, 0, 0, 1) in e["links"],
                     text=b"H\tVN:Z:1.0\n# blocks\nS\t1\t*\tRC:i:20\tLN:i:10\nS\t3\t*\tRC:i:20\tLN:i:10\n# edges\nL\t1\t+\t3\t+\t*\tRC:i:1\nL\t1\t+\t3\t-\t*\tRC:i:1\nL\t1\t-\t3\t+\t*\tRC:i:1\n# paths\n"
                          b"P\tp1\t1+,3+\t*\nP\tp2\t3-,1+\t*\tTP:Z:circular\n")
    return _case(made, pin=lambda e: [s[3] for s in e["segments"]] == [0, 1, 0] and b"S\t2\t*\tRC:i:20\tLN:i:10\tTP:Z:duplicated\n" in e["text"])


def _all_filtered():
    return _case(graph([(True, "A+ B+"), (False, "B-")]), GfaParams(minimum_length=11), pin=lambda e: e["text"] == gfa.HEADER and not e["steps"], text=gfa.HEADER)


def _empty_paths():
    # path 1 was empty before, path 3 (only the short S) becomes empty, path 2 keeps one node
    return _case(graph([(False, ""), (True, "S+ A+"), (True, "S- S+"), (False, "")], lens={"S": 3}), GfaParams(minimum_length=4),
                 pin=lambda e: [p[0] for p in e["paths"]] == [1] and e["links"] == [(0, 0, 0, 0, 1)],
                 text=b"H\tVN:Z:1.0\n# blocks\nS\t1\t*\tRC:i:10\tLN:i:10\n# edges\nL\t1\t+\t1\t+\t*\tRC:i:1\n# paths\nP\tp2\t1+\t*\tTP:Z:circular\n")


def _bridge():
    # A and C become neighbours when the short B between them is filtered: the link A+ C+ is absent from the unfiltered graph
    made = graph([(False, "A+ B+ C+")], lens={"B": 3})
    return _case(made, GfaParams(minimum_length=4), pin=lambda e: e["links"] == [(0, 2, 0, 0, 1)] and
                 (0, 2, 0, 0, 1) not in gfa.gfa_tables(*made[0], GfaParams(), made[1], made[2])["links"],
                 text=b"H\tVN:Z:1.0\n# blocks\nS\t1\t*\tRC:i:10\tLN:i:10\nS\t3\t*\tRC:i:10\tLN:i:10\n# edges\nL\t1\t+\t3\t+\t*\tRC:i:1\n# paths\nP\tp1\t1+,3+\t*\n")


def _sequences(on):
    made = graph([(False, "A+ Z- B+")], lens={"A": 5, "Z": 0, "B": 3})
    a, b = letters(1, 5), letters(2, 3)
    text = (b"H\tVN:Z:1.0\n# blocks\nS\t1\t%s\tRC:i:5\tLN:i:5\nS\t2\t%s\tRC:i:3\tLN:i:3\nS\t3\t%s\tRC:i:0\tLN:i:0\n# edges\nL\t1\t+\t3\t-\t*\tRC:i:1\nL\t2\t-\t3\t+\t*\tRC:i:1\n# paths\n"
            b"P\tp1\t1+,3-,2+\t*\n") % ((a, b, b"") if on else (b"*", b"*", b"*"))
    return _case(made, GfaParams(include_sequences=on), pin=lambda e: (b"S\t3\t\tRC:i:0" in e["text"]) == on, text=text)


# ---------------------------------------------------------------- links
LINKS = {
    "circ_one": ([(True, "A-")], b"L\t1\t+\t1\t+\t*\tRC:i:1\n"),                       # the self link (n, n) of (A-, A-), written A + A +
    "circ_two": ([(True, "A+ B+")], b"L\t1\t+\t2\t+\t*\tRC:i:1\nL\t1\t-\t2\t-\t*\tRC:i:1\n"),   # both directions
    "linear_one": ([(False, "A+")], b""),
    "self_minus": ([(False, "A- A-")], b"L\t1\t+\t1\t+\t*\tRC:i:1\n"),
    "self_mixed": ([(False, "A+ A- A+")], b"L\t1\t+\t1\t-\t*\tRC:i:1\nL\t1\t-\t1\t+\t*\tRC:i:1\n"),
    "both_orientations": ([(False, "A+ B-"), (False, "B+ A-")], b"L\t1\t+\t2\t-\t*\tRC:i:2\n"),
    "two_links_same_blocks": ([(False, "A+ B+"), (False, "A+ B-")], b"L\t1\t+\t2\t+\t*\tRC:i:1\nL\t1\t+\t2\t-\t*\tRC:i:1\n"),
}


def _links(which):
    paths, want = LINKS[which]
    between = lambda t: t[t.index(b"# edges\n") + 8:t.index(b"# paths\n")] if b"# edges\n" in t else b""
    return _case(graph(paths), pin=lambda e: between(e["text"]) == want and len(e["links"]) == want.count(b"L\t"))


def _high_block_index():
    lists, cons, names = graph([(True, "A+ B- C+"), (False, "C+ A+ B-")])
    lists, cons = shift_blocks(lists, cons, (1 << 16) + 5)
    return _case((lists, cons, names), GfaParams(include_sequences=True), pin=lambda e: min(s[0] for s in e["segments"]) > 1 << 16 and min(min(l[:2]) for l in e["links"]) > 1 << 16, json=False)


# ---------------------------------------------------------------- tiles (PGA_EXPORT_TILE_KB=4) and scans
def _padded(make, where, want):
    """make(pad) -> a case whose padding (a consensus or a name `pad` long) lies in front of the item at where(exp): the pad that puts it at `want`"""
    pad = 0
    for _ in range(6):                                                       # (the pad's own decimal widths move the item too)
        at = where(expected_of(make(pad)))
        if at == want:
            break
        pad += want - at
    return make(pad)


def _cut_segment():
    """the second S line starts 3 bytes before the tile edge: "S\\t2" | the rest"""
    make = lambda pad: _case(graph([(False, "A+ B+")], lens={"A": pad}), GfaParams(include_sequences=True), pin=lambda e: e["segments"][1][4] == EDGE - 3)
    return _padded(make, lambda e: e["segments"][1][4], EDGE - 3)


def _cut_link():
    make = lambda pad: _case(graph([(False, "A+ B+")], lens={"A": pad}, ids={"A": 123456, "B": 234567}), GfaParams(include_sequences=True), pin=lambda e: line_at(e, b"L\t") == EDGE - 5)
    return _padded(make, lambda e: line_at(e, b"L\t"), EDGE - 5)


def _cut_step():
    """the second step "234567-" of the P line has its first two digits in front of the tile edge"""
    make = lambda pad: _case(graph([(False, "A+ B- A+")], ids={"A": 123456, "B": 234567}, names=["n" * pad]), pin=lambda e: e["text"].index(b",234567-") + 1 == EDGE - 2)
    return _padded(make, lambda e: e["text"].index(b",234567-") + 1, EDGE - 2)


def _record_end():
    """the tile ends exactly where the last S line ends"""
    make = lambda pad: _case(graph([(False, "A+ B+")], lens={"A": pad}), GfaParams(include_sequences=True), pin=lambda e: line_at(e, b"# edges") == EDGE)
    return _padded(make, lambda e: line_at(e, b"# edges"), EDGE)


def _long_p_line():
    words = " ".join(f"B{k % 7}{'+-'[k % 3 == 0]}" for k in range(2000))
    return _case(graph([(True, words)], ids={f"B{k}": 10000 + k for k in range(7)}), pin=lambda e: len(e["text"]) - e["paths"][0][3] > 2 * EDGE and len(e["steps"]) == 2000)


def _long_consensus():
    return _case(graph([(False, "A+ B+")], lens={"A": 10000, "B": 5000}), GfaParams(include_sequences=True), pin=lambda e: e["segments"][0][4] < EDGE and e["segments"][1][4] > 2 * EDGE)


def _long_name():
    return _case(graph([(False, "A+"), (False, "A-")], names=["x" * 9000, "y" * 5000]), pin=lambda e: e["paths"][0][3] < EDGE and e["paths"][1][3] > 2 * EDGE and len(e["text"]) > 3 * EDGE)


def _path_of(n):
    """one circular path of n nodes over three blocks, and a short one behind it"""
    words = " ".join(f"B{(k * k) % 3}{'+-'[k % 2]}" for k in range(n))
    return _case(graph([(True, words), (False, "B0+ B1+")]), GfaParams(maximum_depth=10 ** 9), pin=lambda e: e["paths"][0][1] == n and e["paths"][1][2] == n)


@functools.lru_cache(maxsize=None)
def second_level():
    """past the second level of the tile scan: 1024 * 1024 + 1 nodes on four blocks and three paths, include_sequences off -> (arrays, exp):
    the three input arrays as numpy records, and gfa_tables of the same lists"""
    n = TILE * TILE + 1
    k = np.arange(n, dtype=np.uint64)
    nodes = np.zeros(n, NP_NODE)
    nodes["node_id"] = k + 101
    nodes["block"] = (k * k + k // 5) % 4
    nodes["reverse"] = (k // 3) % 2
    bounds = [0, 5, TILE * SCAN_THREADS + 3, n]
    for b in range(4):
        at = np.flatnonzero(nodes["block"] == b)
        nodes["member"][at] = np.arange(len(at))
    depth = np.bincount(nodes["block"], minlength=4)
    blocks = np.array([(7 + 10 * b, 10 + b, depth[b], 1, 0) for b in range(4)], NP_BLOCK)
    paths = np.array([(p + 1, bounds[p], bounds[p + 1] - bounds[p], p % 2) for p in range(3)], NP_PATH)
    lists = ([tuple(r)[:4] for r in blocks.tolist()], [tuple(r) for r in paths.tolist()], [tuple(r)[:6] for r in nodes.tolist()])
    names = [b"first", b"second", b"third"]
    exp = gfa.gfa_tables(*lists, GfaParams(minimum_length=11), None, names)
    return {"blocks": blocks, "paths": paths, "nodes": nodes, "names": names, "params": GfaParams(minimum_length=11)}, exp


CASES = {
    "width_ids": _width_ids, "width_counts": _width_counts, "rc_above_2_32": _rc_above_2_32, "names": _names,
    **{f"bounds_{k}": functools.partial(_bounds, k) for k in BOUNDS},
    "no_duplicated_on": functools.partial(_no_duplicated, True), "no_duplicated_off": functools.partial(_no_duplicated, False),
    "all_filtered": _all_filtered, "empty_paths": _empty_paths, "bridge": _bridge,
    "sequences_on": functools.partial(_sequences, True), "sequences_off": functools.partial(_sequences, False),
    **{f"links_{k}": functools.partial(_links, k) for k in LINKS},
    "high_block_index": _high_block_index,
    "cut_segment": _cut_segment, "cut_link": _cut_link, "cut_step": _cut_step, "record_end": _record_end,
    "long_p_line": _long_p_line, "long_consensus": _long_consensus, "long_name": _long_name,
    **{f"path_{n}": functools.partial(_path_of, n) for n in (TILE - 1, TILE, TILE + 1)},
}


def expected_of(c):
    return gfa.gfa_tables(*c["lists"], c["params"], c["cons"], c["names"])


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_of(case(name))


# ---------------------------------------------------------------- seeded random graphs
PARAM_SETS = (dict(), dict(include_sequences=True), dict(minimum_length=8, maximum_depth=3), dict(no_duplicated=True, minimum_depth=2, include_sequences=True))


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """2-12 paths over 5-60 blocks, mixed strands and circularity, block ids of mixed widths, some blocks visited twice by a path"""
    rng = random.Random(1000 + seed)
    n_blocks, n_paths = rng.randint(5, 60), rng.randint(2, 12)
    words = [f"B{k:02d}" for k in range(n_blocks)]
    ids = dict(zip(words, sorted(rng.sample(range(1, 5000), n_blocks - 2) + [rng.getrandbits(64), rng.getrandbits(40)])))
    lens = {w: rng.choice((0, 1, 5, 8, 8, 13, 40, 200)) for w in words}
    paths = [(rng.random() < 0.5, " ".join(rng.choice(words) + rng.choice("+-") for _ in range(rng.choice((0, 1, 2, 5, 9, 30))))) for _ in range(n_paths)]
    used = {w[:-1] for _, s in paths for w in s.split()}
    lists, cons, names = graph(paths, lens={w: n for w, n in lens.items() if w in used}, ids={w: i for w, i in ids.items() if w in used},
                               names=[f"path {k} é" * (k % 3) for k in range(n_paths)])
    return {"lists": lists, "cons": cons, "names": names, "json": True}


# ---------------------------------------------------------------- the arguments of the call, through numpy
def pack(lists, cons, names):
    """-> (graph_args, cons, names, what must stay alive)"""
    blocks, paths, nodes = lists
    B = np.array([(b[0], b[1], b[2], 1 if b[3] else 0, 0) for b in blocks], NP_BLOCK)
    P = np.array([tuple(p) for p in paths], NP_PATH) if paths else np.zeros(0, NP_PATH)
    N = np.array([(n[0], n[1], n[2], n[3], n[4], 1 if n[5] else 0, 0) for n in nodes], NP_NODE) if nodes else np.zeros(0, NP_NODE)
    return pack_arrays(B, P, N), cons, names, (B, P, N)


def pack_arrays(B, P, N):
    ptr = lambda a: C.c_void_p(a.ctypes.data) if len(a) else None
    return (len(B), ptr(B), len(P), ptr(P), len(N), ptr(N))


def view(ptr, dtype, n):
    return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(C.cast(ptr, C.c_void_p).value), dtype, n) if n else np.zeros(0, dtype)
