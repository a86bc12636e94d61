"""Graphs for pga_remove_paths (pangraph_amd/remove.py) and the expectation they are held against: `host_remove`, built from
pangraph_amd.simplify.remove_path (which tests/test_simplify_cpu.py holds to the reference's own vector) applied path by path to the dict
graph.  Which members, nodes, paths and blocks survive, and every edit of the survivors, come from that function; the flat layout of the
answer (offsets, maps, counts) is the input's arrays filtered by what survived.  Every graph is built so that the structure a test aims
at exists by construction; tests/test_remove_cpu.py pins each of them, so a generator that stops producing its case fails there and not
silently on the GPU.

A case is {"lists": (blocks, paths, nodes) as topology.pack_lists takes them, "dicts": per block index {"consensus", "members": [edit]} in
slot order (a dead block has no member), "keep": one truth value per path, "letters": None or (ins_seq bytes, [seq_off per insertion]) to
replace what the packing lays out}."""
import copy
import ctypes as C
import functools
import json
import os
import random

import numpy as np

import simplify_gen as sg
import topo_gen as tg
from pangraph_amd import remove as rm
from pangraph_amd import simplify as sp
from pangraph_amd import topology as tp
from pangraph_amd.mapvar import del_t, ins_t, sub_t
from pangraph_amd.reconsensus import rc_member_t
from pangraph_amd.reconstruct import _Packed

TILE = tp.TILE                           # members per workgroup of the member scan (RM_TILE of pga_remove_idx.h)
SCAN_THREADS = 256                       # threads of the one workgroup that scans the tile sums (RM_THREADS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT_FIELDS = ("blocks", "paths", "nodes", "rc_blocks", "members", "subs", "dels", "inss", "ins_seq", "member_map", "path_map", "counts", "dicts")
STRAND = "+-"


# ---------------------------------------------------------------- lists and dicts <-> the dict shape of simplify.normalize
def to_graph(lists, dicts):
    """-> (g, order, bids): the dict graph of the alive blocks, the member order of each, the id of every block index; path k is named "p<id>" """
    blocks, paths, nodes = lists
    bids = [b[0] for b in blocks]
    g = {"paths": {}, "nodes": {}, "blocks": {b[0]: {"consensus": dicts[i]["consensus"], "alignments": {}} for i, b in enumerate(blocks) if b[3]}}
    order = {b[0]: [None] * b[2] for b in blocks if b[3]}
    for pid, off, n, circular in paths:
        g["paths"][pid] = {"nodes": [x[0] for x in nodes[off:off + n]], "tot_len": 0, "circular": bool(circular), "name": f"p{pid}"}
        for nid, pos0, pos1, b, member, rev in nodes[off:off + n]:
            g["nodes"][nid] = {"block_id": bids[b], "path_id": pid, "strand": STRAND[1 if rev else 0], "position": (pos0, pos1)}
            g["blocks"][bids[b]]["alignments"][nid] = dicts[b]["members"][member]
            order[bids[b]][member] = nid
    return g, order, bids


def pack(case):
    """-> (graph args, block args, ins_seq_len, what keeps them alive)"""
    args = tp.pack_lists(*case["lists"])
    K = _Packed(case["dicts"], [])
    n_letters = C.sizeof(K.L)
    if case.get("letters"):
        seq, offs = case["letters"]
        for k, off in enumerate(offs):
            K.I[k].seq_off = off
        K.L = C.create_string_buffer(bytes(seq), max(len(seq), 1))
        n_letters = len(seq)
    return args, K.args()[:7], n_letters, K


def flat_of(case):
    """the block arrays as lists: (members [(n_subs, n_dels, n_inss)], subs [(pos, alt)], dels [(pos, len)], inss [(pos, len, seq_off)], ins_seq bytes)"""
    _, (_, _, M, S, D, I, L), n_letters, K = pack(case)
    members = [(M[m].n_subs, M[m].n_dels, M[m].n_inss) for m in range(K.n_mem)]
    ns, nd, ni = (sum(m[k] for m in members) for k in range(3))
    return (members, [(S[k].pos, S[k].alt) for k in range(ns)], [(D[k].pos, D[k].len) for k in range(nd)], [(I[k].pos, I[k].len, I[k].seq_off) for k in range(ni)], bytes(L.raw[:n_letters]))


def host_remove(case, flags=0):
    """what RemoveOut.to_lists() gives, plus "dicts" (to_dicts()), from simplify.remove_path applied to every path that is not kept"""
    blocks, paths, nodes = case["lists"]
    dicts, keep = case["dicts"], case["keep"]
    g, order, bids = to_graph(case["lists"], dicts)
    removed = [p[0] for p, k in zip(paths, keep) if not k]
    for pid in removed:
        sp.remove_path(g, pid)
    # (an alive block without a node is no graph of the reference's; remove_path would drop it only when some path goes)
    assert all(b[2] for b in blocks if b[3])
    index = {b[0]: i for i, b in enumerate(blocks) if b[3]}
    after = {bid: [n for n in order[bid] if n in g["nodes"]] for bid in order}
    assert all((bid in g["blocks"]) == bool(after[bid]) and (bid not in g["blocks"] or sorted(g["blocks"][bid]["alignments"]) == sorted(after[bid])) for bid in order)
    slot = {n: k for ids in after.values() for k, n in enumerate(ids)}
    exp = {"blocks": [(b[0], b[1], len(after[b[0]]), 1) if b[3] and b[0] in g["blocks"] else (b[0], 0, 0, 0) for b in blocks], "paths": [], "nodes": [], "path_map": []}
    for (pid, _, _, circular), k in zip(paths, keep):
        exp["path_map"].append(len(exp["paths"]) if k else -1)
        if not k:
            assert pid not in g["paths"]
            continue
        ids = g["paths"][pid]["nodes"]
        exp["paths"].append((pid, len(exp["nodes"]), len(ids), circular))
        for n in ids:
            x = g["nodes"][n]
            exp["nodes"].append((n, x["position"][0], x["position"][1], index[x["block_id"]], slot[n], int(x["strand"] == "-")))
    exp["dicts"] = [{"consensus": dicts[i]["consensus"], "members": [g["blocks"][b[0]]["alignments"][n] for n in after[b[0]]] if b[3] and b[0] in g["blocks"] else []} for i, b in enumerate(blocks)]
    exp["rc_blocks"] = [(len(dicts[i]["consensus"]), len(exp["dicts"][i]["members"])) for i in range(len(blocks))]
    # the flat layout: the input's arrays filtered by what survived
    kept = [n in g["nodes"] for b in blocks if b[3] for n in order[b[0]]]
    members, subs, dels, inss, seq = flat_of(case)
    assert len(kept) == len(members)
    exp.update(members=[], subs=[], dels=[], inss=[], member_map=[])
    letters = bytearray()
    s = d = i = 0
    for m, (ns, nd, ni) in enumerate(members):
        exp["member_map"].append(len(exp["members"]) if kept[m] else -1)
        if kept[m]:
            exp["members"].append((ns, nd, ni))
            exp["subs"] += subs[s:s + ns]; exp["dels"] += dels[d:d + nd]
            for pos, ln, off in inss[i:i + ni]:
                if flags & rm.COMPACT_LETTERS:
                    exp["inss"].append((pos, ln, len(letters)))
                    letters += seq[off:off + ln]
                else:
                    exp["inss"].append((pos, ln, off))
        s += ns; d += nd; i += ni
    exp["ins_seq"] = bytes(letters) if flags & rm.COMPACT_LETTERS else None
    exp["counts"] = (len(blocks), len(exp["paths"]), len(exp["nodes"]), len(exp["members"]), sum(1 for b in exp["blocks"] if not b[3]),
                     len(exp["subs"]), len(exp["dels"]), len(exp["inss"]), len(letters))
    return exp


def graph_after(case):
    """the dict graph behind the removal (remove_path alone)"""
    g, _, _ = to_graph(case["lists"], case["dicts"])
    for p, k in zip(case["lists"][1], case["keep"]):
        if not k:
            sp.remove_path(g, p[0])
    return g


# ---------------------------------------------------------------- members
def make_case(lists, keep, seed=0, member=None, cons=None):
    """member(block index, slot, cons_len, rng) -> an edit, or None for a small sorted one"""
    rng = random.Random(seed)
    dicts = []
    for i, (bid, cons_len, depth, alive) in enumerate(lists[0]):
        L = cons_len
        mem = []
        for k in range(depth if alive else 0):
            e = member(i, k, L, rng) if member else None
            mem.append(e if e is not None else sg._sorted_member(rng, L, min(L, rng.randint(0, 3)), min(L, rng.randint(0, 2)), rng.randint(0, 2)))
        dicts.append({"consensus": sg._letters(rng, L), "members": mem})
    assert len(keep) == len(lists[1])
    return {"lists": lists, "dicts": dicts, "keep": [bool(k) for k in keep], "letters": None}


def with_dead(lists, at, entry=(77, 7, 3, 0)):
    """the same graph with a dead block entry before block index `at`"""
    blocks, paths, nodes = lists
    return (blocks[:at] + [entry] + blocks[at:], paths, [(n[0], n[1], n[2], n[3] + (n[3] >= at), n[4], n[5]) for n in nodes])


def reference_case():
    v = json.load(open(os.path.join(GOLDEN, "simplify_vectors.json")))["simplify_run"]
    g = sp.normalize(v["graph"])
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    lists = tg.to_lists(g, order)
    dicts = [{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in sorted(g["blocks"])]
    return {"lists": lists, "dicts": dicts, "keep": [pid != v["remove_path"] for pid in sorted(g["paths"])], "letters": None, "graph": g}


def tile_case(n):
    """n members in all: a deep block F whose members are kept, removed, kept in three runs, and a block Z with one removed and one kept
    member at the very end (global members n - 2 and n - 1)"""
    a, b = (n - 2) // 3, (n - 2) // 3 + 1
    c = n - 2 - a - b
    lists = tg.graph([(False, " ".join(["F+"] * a + ["Z+"])), (True, " ".join(["F-"] * b + ["Z-"])), (False, " ".join(["F+"] * c))], lens={"F": 30, "Z": 12})
    return make_case(lists, [1, 0, 1], seed=n, member=lambda i, k, L, rng: sg._sorted_member(rng, L, k % 3, k % 2, (k + 1) % 2, ins_len=1 + k % 5))


def skew_case():
    """block A: a kept member with 5 000 substitutions and 3 000 insertions, 1 000 kept members without an edit, a removed member with the
    same long lists, 1 000 removed members without an edit"""
    lists = tg.graph([(False, " ".join(["A+"] * 1001)), (False, " ".join(["A-"] * 1001))], lens={"A": 6000})
    long_one = lambda i, k, L, rng: sg._sorted_member(rng, L, 5000, 7, 3000) if k in (0, 1001) else copy.deepcopy(tg.EDIT)
    return make_case(lists, [1, 0], seed=5, member=long_one)


def offsets_case():
    """six blocks of two members: a removed one with lists of 3, 5 and 7 entries, then a kept one whose three lists have one of LIST_LENGTHS"""
    names = " ".join(f"B{k}+" for k in range(6))
    lists = tg.graph([(False, names), (True, names)], lens={f"B{k}": 200 for k in range(6)})
    return make_case(lists, [0, 1], seed=9, member=lambda i, k, L, rng: sg._sorted_member(rng, L, 3, 5, 7) if k == 0 else sg._sorted_member(rng, L, *[sg.LIST_LENGTHS[i]] * 3))


def letters_case():
    """block A, three members (kept, removed, kept), each with insertions of every length of INS_LENGTHS; the letters lie in shuffled order
    with gaps between them, and the first and the last kept insertion of length 15 share theirs"""
    lists = tg.graph([(False, "A+"), (False, "A+"), (True, "A-")], lens={"A": 50})
    rng = random.Random(11)
    c = make_case(lists, [1, 0, 1], seed=11, member=lambda i, k, L, rng: dict(sg._sorted_member(rng, L, 2, 1, 0), inss=[(7 * j, sg._letters(rng, n)) for j, n in enumerate(sg.INS_LENGTHS)]))
    shared = c["dicts"][0]["members"][0]["inss"][1][1]
    c["dicts"][0]["members"][2]["inss"][1] = (c["dicts"][0]["members"][2]["inss"][1][0], shared)
    flat = [seq for m in c["dicts"][0]["members"] for _, seq in m["inss"]]
    place = list(range(len(flat)))
    rng.shuffle(place)
    buf, offs = bytearray(b"nn"), [None] * len(flat)
    for k in place:
        if k == 11:                                                   # (member 2's insertion of 15 letters: the letters of member 0's)
            continue
        offs[k] = len(buf)
        buf += flat[k].encode() + b"n" * (k % 3)
    offs[11] = offs[1]
    c["letters"] = (bytes(buf), offs)
    return c


def high_index_case():
    base = CASES["one_block_twice"]()
    lists = tg.shift_blocks(base["lists"], (1 << 16) + 5)
    return dict(base, lists=lists, dicts=[{"consensus": "", "members": []}] * ((1 << 16) + 5) + base["dicts"])


CASES = {
    "reference": reference_case,
    "keep_all": lambda: make_case(tg.graph([(True, "A+ B- C+"), (False, "C+ A+ B-"), (False, "B+")]), [1, 1, 1], seed=1),
    "keep_none": lambda: make_case(tg.graph([(True, "A+ B- C+"), (False, "C+ A+ B-"), (False, "B+")]), [0, 0, 0], seed=2),
    # a removed path and a kept path without a node
    "empty_path": lambda: make_case(tg.graph([(False, ""), (False, "A+ B+"), (True, ""), (False, "B- A+")]), [0, 1, 1, 0], seed=3),
    # path 1 (removed) has two nodes in A; A also holds a node of the kept path 2
    "one_block_twice": lambda: make_case(tg.graph([(False, "A+ B+ A-"), (False, "A+ C+")]), [0, 1], seed=4),
    # B lies on the removed path only, between the survivors A and C
    "dies": lambda: make_case(tg.graph([(False, "A+ B+ C+"), (False, "A+ C-")]), [0, 1], seed=6),
    "dead_before": lambda: make_case(with_dead(tg.graph([(False, "A+ B+ C+"), (False, "A+ C-"), (True, "B- B+")]), 1), [1, 0, 1], seed=7),
    # the removed path is circular: its wrap (C -> A) lies in blocks that the kept path holds too
    "wrap_node": lambda: make_case(tg.graph([(True, "A+ B+ C+"), (False, "C+ A-")]), [0, 1], seed=8),
    f"tile_{TILE - 1}": lambda: tile_case(TILE - 1),
    f"tile_{TILE}": lambda: tile_case(TILE),
    f"tile_{TILE + 1}": lambda: tile_case(TILE + 1),
    "skew": skew_case,
    "offsets": offsets_case,
    "letters": letters_case,
    "high_block_index": high_index_case,
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def expected(name, flags=0):
    return host_remove(case(name), flags)


@functools.lru_cache(maxsize=None)
def random_case(seed):
    """tg.random_graph with random members and a random keep mask; every third graph carries a dead entry, every fourth its letters in reversed order"""
    rng = random.Random(4000 + seed)
    lists = tg.random_graph(seed)
    if seed % 3 == 0:
        lists = with_dead(lists, rng.randrange(len(lists[0]) + 1), (rng.randrange(500), 9, 2, 0))
    keep = [rng.random() < 0.5 for _ in lists[1]]
    c = make_case(lists, keep, seed=4000 + seed, member=lambda i, k, L, r: sg._random_member(r, L))
    if seed % 4 == 0:
        _, _, _, inss, seq = flat_of(c)
        c["letters"] = (bytes(reversed_segments(seq, inss)), [len(seq) - off - ln + 2 for _, ln, off in inss])
    return c


def reversed_segments(seq, inss):
    """the letter buffer in which insertion k's letters lie at len(seq) - off - len + 2 (the segments in reversed order, two bytes of padding first)"""
    out = bytearray(b"x" * (len(seq) + 2))
    for _, ln, off in inss:
        at = len(seq) - off - ln + 2
        out[at:at + ln] = seq[off:off + ln]
    return out[:len(seq) + 2]


# ---------------------------------------------------------------- past the second level of the tile scan: numpy arrays in, numpy arrays expected
NP_NODE, NP_PATH, NP_BLOCK = np.dtype(tp.topo_node_t), np.dtype(tp.topo_path_t), np.dtype(tp.topo_block_t)
NP_MEMBER, NP_SUB, NP_DEL, NP_INS = np.dtype(rc_member_t), np.dtype(sub_t), np.dtype(del_t), np.dtype(ins_t)
NP_RC = np.dtype([("consensus", "<u8"), ("cons_len", "<u4"), ("n_members", "<u4")])          # (pga_rc_block_t with its pointer as a number)


@functools.lru_cache(maxsize=None)
def second_level(n=TILE * SCAN_THREADS + 40):
    """n members (a multiple of 4) in four blocks, node i in block i % 4 at slot i // 4; five paths of which the second and the fourth go (the fourth ends a few members behind the edge of the second level).
    Member m has m % 3 substitutions, a deletion when m % 5 == 0 and an insertion of 1 + m % 8 letters when m % 7 == 0.
    -> (inputs, expected): dicts of numpy arrays; expected["kept"] is the mask over the input members"""
    assert n % 4 == 0
    q = n // 4
    i = np.arange(n)
    rest = n - (n // 2 - 1) - 3 - n // 4
    sizes = [n // 2 - 1, 3, n // 4, rest - min(60, rest // 2), min(60, rest // 2)]
    keep = np.array([1, 0, 1, 0, 1], np.uint8)
    N = np.zeros(n, NP_NODE)
    N["node_id"], N["block"], N["member"], N["reverse"] = 10 + i, i % 4, i // 4, (i // 3) % 2
    N["pos0"], N["pos1"] = 7 * i, 7 * i + 5
    P = np.zeros(5, NP_PATH)
    P["path_id"], P["n_nodes"], P["circular"] = [3, 5, 8, 9, 12], sizes, [0, 1, 0, 1, 0]
    P["node_off"] = np.concatenate(([0], np.cumsum(sizes)[:-1]))
    B = np.zeros(4, NP_BLOCK)
    B["block_id"], B["cons_len"], B["depth"], B["alive"] = [11, 12, 13, 14], 40, q, 1
    cons = np.frombuffer(b"ACGT" * 10, np.uint8).copy()
    R = np.zeros(4, NP_RC)
    R["consensus"], R["cons_len"], R["n_members"] = cons.ctypes.data, 40, q
    m = np.arange(n)
    M = np.zeros(n, NP_MEMBER)
    M["n_subs"], M["n_dels"], M["n_inss"] = m % 3, m % 5 == 0, m % 7 == 0
    owner = lambda cnt: np.repeat(m, cnt)
    so, do, io = owner(M["n_subs"]), owner(M["n_dels"]), owner(M["n_inss"])
    S = np.zeros(len(so), NP_SUB); S["pos"], S["alt"] = so % 40, 65 + so % 20
    D = np.zeros(len(do), NP_DEL); D["pos"], D["len"] = do % 39, 1
    I = np.zeros(len(io), NP_INS); I["pos"], I["len"], I["seq_off"] = io % 41, 1 + io % 8, io % 32
    seq = np.frombuffer((b"ACGTTGCA" * 5), np.uint8).copy()
    inputs = {"blocks": B, "paths": P, "nodes": N, "rc_blocks": R, "members": M, "subs": S, "dels": D, "inss": I, "ins_seq": seq, "keep": keep, "cons": cons}
    path_of = np.repeat(np.arange(5), sizes)
    node_kept = keep[path_of] != 0
    g = (i % 4) * q + i // 4                                       # the global member of node i
    kept = np.zeros(n, bool)
    kept[g] = node_kept
    rank = np.cumsum(kept) - kept                                    # kept members before m
    first_rank = rank[np.arange(4) * q]
    oN = N[node_kept].copy()
    oN["member"] = rank[g[node_kept]] - first_rank[oN["block"]]
    oP = P[keep != 0].copy()
    oP["node_off"] = np.concatenate(([0], np.cumsum(oP["n_nodes"])[:-1]))
    oB = B.copy()
    oB["depth"] = [kept[b * q:(b + 1) * q].sum() for b in range(4)]
    oR = R.copy(); oR["n_members"] = oB["depth"]
    oI = I[kept[io]].copy()
    cI = oI.copy()
    cI["seq_off"] = np.cumsum(oI["len"]) - oI["len"]
    gather = np.repeat(oI["seq_off"].astype(np.int64) - cI["seq_off"].astype(np.int64), oI["len"]) + np.arange(int(oI["len"].sum()))
    expected = {"kept": kept, "blocks": oB, "paths": oP, "nodes": oN, "rc_blocks": oR, "members": M[kept], "subs": S[kept[so]], "dels": D[kept[do]], "inss": oI,
                "inss_compact": cI, "ins_seq": seq[gather], "member_map": np.where(kept, rank, -1).astype(np.int64), "path_map": np.array([0, -1, 1, -1, 2], np.int32)}
    return inputs, expected


def second_level_case(n):
    """the same graph as a case of lists and dicts (small n only): what ties the numpy expectation to host_remove"""
    inp, _ = second_level(n)
    lists = ([(int(b["block_id"]), int(b["cons_len"]), int(b["depth"]), 1) for b in inp["blocks"]],
             [(int(p["path_id"]), int(p["node_off"]), int(p["n_nodes"]), int(p["circular"])) for p in inp["paths"]],
             [(int(x["node_id"]), int(x["pos0"]), int(x["pos1"]), int(x["block"]), int(x["member"]), int(x["reverse"])) for x in inp["nodes"]])
    seq = bytes(inp["ins_seq"])
    S, D, I = inp["subs"], inp["dels"], inp["inss"]
    dicts, s, d, i, m = [], 0, 0, 0, 0
    for b in inp["blocks"]:
        mem = []
        for _ in range(int(b["depth"])):
            c = inp["members"][m]
            mem.append({"subs": [(int(x["pos"]), chr(int(x["alt"]))) for x in S[s:s + c["n_subs"]]], "dels": [(int(x["pos"]), int(x["len"])) for x in D[d:d + c["n_dels"]]],
                        "inss": [(int(x["pos"]), seq[int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])].decode()) for x in I[i:i + c["n_inss"]]]})
            s += c["n_subs"]; d += c["n_dels"]; i += c["n_inss"]; m += 1
        dicts.append({"consensus": bytes(inp["cons"]).decode(), "members": mem})
    return {"lists": lists, "dicts": dicts, "keep": [bool(k) for k in inp["keep"]], "letters": (seq, [int(x) for x in I["seq_off"]])}
