"""Cuts for pga_apply_merge (pangraph_amd/apply.py) and the expectation they are held against: `host_apply`, the output of one call computed
from the host reweave() of pangraph_amd/reweave.py (update=None) -- the graph behind it, with the merged blocks put in as graph_merging.rs:
156-165 does, re-packed with topology.pack_graph; new_nodes, member_src and the block records read off the dicts.  The reference vector and
the random graphs go through reweave_ref / slice_ref; a written-out case hands reweave() its plan and its slices directly (reweave's plan= and
slicer= stand-ins), so that the structure it aims at exists by construction.  tests/test_apply_cpu.py pins every case on the host side.

A case is {"args": (blocks, paths, nodes, cut, intervals, slices, members) as apply.apply_merge takes them, "exp": what it returns,
"after": the dict graph behind the call, "before": the one in front of it}."""
import functools
import json
import os
import random

import reweave_gen as rg
import reweave_ref as rr
import slice_ref as sr
import topo_gen as tg
from pangraph_amd import reweave as rw
from pangraph_amd import simplify as sp
from pangraph_amd import topology as tp

NONE = 0xFFFFFFFF
TILE = tp.TILE
SCAN_THREADS = 256                       # threads of the one workgroup that scans the tile sums (TP_THREADS of pga_topo_idx.h)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUT_FIELDS = ("new_nodes", "old_node", "new_blocks", "member_src", "block_map", "blocks", "paths", "nodes")


def ref_slicer(bl):
    return sr.slice_blocks([dict(b, intervals=[sr.interval(s, e, bool(f), False, bool(f)) for s, e, f in b["intervals"]]) for b in bl])


def lists_of(g, order):
    """what topology.unpack_lists(topology.pack_graph(g, order)) gives, without the C arrays in between (tests/test_apply_cpu.py holds the two
    against each other): the largest case has a quarter of a million nodes"""
    bids = sorted(g["blocks"])
    at = {b: i for i, b in enumerate(bids)}
    slot = {n: k for b in bids for k, n in enumerate(order[b])}
    paths, nodes = [], []
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        paths.append((pid, len(nodes), len(p["nodes"]), int(bool(p["circular"]))))
        for nid in p["nodes"]:
            n = g["nodes"][nid]
            nodes.append((nid, n["position"][0], n["position"][1], at[n["block_id"]], slot[nid], int(n["strand"] == "-")))
    return [(b, len(g["blocks"][b]["consensus"]), len(order[b]), 1) for b in bids], paths, nodes


# ---------------------------------------------------------------- the expectation
def host_apply(g, matches, plan, slicer, thr=rg.THR, shift=0):
    """g: a graph in the shape of simplify.normalize (not changed); matches, plan, slicer, thr: what reweave() takes; shift: the number of dead
    entries put in front of the block table -> the case"""
    order_in = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    blocks, paths, nodes = lists_of(g, order_in)
    seen = {}

    def plan_(groups, ms, t):
        seen["p"], seen["bids"] = plan(groups, ms, t), [b["block_id"] for b in groups[0]]
        return seen["p"]

    def slicer_(bl):
        seen["rows"] = slicer(bl)
        return seen["rows"]

    # (reweave changes the three maps and the paths' node lists, never a node or a block that stays: those are shared with g)
    mine = {"paths": {k: dict(v, nodes=list(v["nodes"])) for k, v in g["paths"].items()}, "nodes": dict(g["nodes"]), "blocks": dict(g["blocks"])}
    after, promises = rw.reweave(mine, matches, thr, plan=plan_, slicer=slicer_)
    p, bids, rows = seen["p"], seen["bids"], seen["rows"]
    for q in promises:                                                         # graph_merging.rs:156-165 (the blocks as they stand before solve_promise)
        assert q["new_block_id"] not in after["blocks"] and not set(q["anchor"]["alignments"]) & set(q["append"]["alignments"])
        after["blocks"][q["new_block_id"]] = {"consensus": q["anchor"]["consensus"], "alignments": {**q["anchor"]["alignments"], **q["append"]["alignments"]}}
    at_in = {b[0]: i for i, b in enumerate(blocks)}
    cut = [(at_in[bids[b["block"]]] + shift, b["n_intervals"], b["first_interval"]) for b in p["blocks"]]
    slices, members, k_of, new_nodes, old_node = [], [], {}, [], []
    order_after = {b: sorted(blk["alignments"]) for b, blk in after["blocks"].items()}
    at_after = {b: i for i, b in enumerate(sorted(after["blocks"]))}
    slot = {n: k for ids in order_after.values() for k, n in enumerate(ids)}
    for b, per_iv in zip(p["blocks"], rows):
        olds = order_in[bids[b["block"]]]
        for j, r in enumerate(per_iv):
            iv = p["intervals"][b["first_interval"] + j]
            slices.append((len(members), len(r["kept"]), len(r["dropped"])))
            for m in r["kept"]:
                nid = sp.node_id(iv["new_block_id"], g["nodes"][olds[m["member"]]]["path_id"], m["reverse"], m["pos"])
                x = after["nodes"][nid]
                assert x["block_id"] == iv["new_block_id"] and nid not in k_of
                k_of[nid] = len(members)
                members.append((m["member"], int(m["reverse"]), m["pos"][0], m["pos"][1]))
                new_nodes.append((nid, x["position"][0], x["position"][1], at_after[x["block_id"]], slot[nid], int(x["strand"] == "-")))
                old_node.append(olds[m["member"]])
    made = {}                                                                  # new block id -> [kind, interval_a, interval_b]
    for s, iv in enumerate(p["intervals"]):
        if not iv["aligned"]:
            made[iv["new_block_id"]] = [0, s, 0]
        else:
            made.setdefault(iv["new_block_id"], [1, 0, 0])[1 if iv["is_anchor"] else 2] = s
    new_blocks, member_src = [], []
    for bid in sorted(made):
        new_blocks.append((at_after[bid], *made[bid], len(member_src)))
        member_src += [k_of[n] for n in order_after[bid]]
    exp = {"new_nodes": new_nodes, "old_node": old_node, "new_blocks": new_blocks, "member_src": member_src, "block_map": [], "blocks": None, "paths": None, "nodes": None}
    if cut:
        gone = {bids[b["block"]] for b in p["blocks"]}
        exp["block_map"] = [NONE] * shift + [NONE if b[0] in gone else at_after[b[0]] for b in blocks]
        exp["blocks"], exp["paths"], exp["nodes"] = lists_of(after, order_after)
    if shift:
        blocks, paths, nodes = tg.shift_blocks((blocks, paths, nodes), shift)
    ivs = list(p["intervals"] or [])
    return {"args": (blocks, paths, nodes, cut, ivs, slices, members), "exp": exp, "before": g, "after": after, "promises": promises}


# ---------------------------------------------------------------- cuts written out
def synth(lists, cuts, drop=lambda bid, member, interval: False, shift=0):
    """synth_graph on the lists of topo_gen.graph"""
    return synth_graph(tg.to_graph(*lists)[0], cuts, drop, shift)


def synth_graph(g, cuts, drop=lambda bid, member, interval: False, shift=0):
    """g: a dict graph; cuts: {block id: [(start, end, new block id, aligned, is_anchor)]}; drop: which members a slice leaves out.  A kept
    member keeps its old strand and lies at (old pos0 + start, old pos0 + end)."""
    bids = sorted(cuts)
    p = {"n_failed": 0, "blocks": [], "intervals": [], "slice_intervals": [], "promises": []}
    rows = []
    for k, bid in enumerate(bids):
        p["blocks"].append({"block": k, "n_intervals": len(cuts[bid]), "first_interval": len(p["intervals"]), "status": 0, "fail_interval": -1})
        per = []
        for j, (start, end, new_id, aligned, anchor) in enumerate(cuts[bid]):
            p["intervals"].append({"start": start, "end": end, "aligned": int(aligned), "new_block_id": new_id, "is_anchor": int(anchor), "reverse": 0, "match": -1,
                                   "extend_left": 0, "extend_right": 0})
            p["slice_intervals"].append((start, end, 0))
            kept, dropped = [], []
            for m, n in enumerate(sorted(g["blocks"][bid]["alignments"])):
                o = g["nodes"][n]
                if drop(bid, m, j):
                    dropped.append(m)
                else:
                    kept.append(dict(member=m, reverse=o["strand"] == "-", node=(start, end), pos=(o["position"][0] + start, o["position"][0] + end), subs=[], dels=[], inss=[]))
            per.append({"kept": kept, "dropped": dropped})
        rows.append(per)
    for new_id in sorted({iv["new_block_id"] for iv in p["intervals"] if iv["aligned"]}):
        p["promises"].append({"new_block_id": new_id, "reverse": 0, "cigar": []})
    return host_apply(g, [{"qry": b, "ref": b} for b in bids], lambda *a: p, lambda bl: rows, shift=shift)


def pieces(n, length, first_id):
    """n unaligned intervals that tile [0, n * length)"""
    return [(k * length, (k + 1) * length, first_id + k, False, False) for k in range(n)]


def tile_case(n_before):
    """a cut node that expands to 5 nodes behind n_before positions that stay"""
    lists = tg.graph([(False, " ".join(["F+"] * n_before + ["X+", "F-"]))], lens={"F": 4, "X": 50})
    return synth(lists, {2: pieces(5, 10, 7000)})


@functools.lru_cache(maxsize=None)
def second_level_case():
    """more positions than one workgroup scans tile sums for in one pass: cut nodes at the first position, on both sides of that edge, and at the last"""
    n = TILE * SCAN_THREADS
    spots = (0, n - 1, n, n + 39)                                              # block X (id 2, 20 letters); everything else is F (id 1, 3 letters)
    nodes, f = [], 0
    for at in range(n + 40):
        k = spots.index(at) if at in spots else -1
        nodes.append((101 + at, 4 * at, 4 * at + 3, 0, f, 0) if k < 0 else (101 + at, 4 * at, 4 * at + 20, 1, k, int(at == n)))
        f += k < 0
    return synth(([(1, 3, f, 1), (2, 20, 4, 1)], [(1, 0, n + 40, 1)], nodes), {2: pieces(2, 10, 9000)})


def _reference():
    vec = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
    g, matches = rg.reference_graph(vec)
    return host_apply(g, matches, rr.expected_call, ref_slicer, thr=vec["reweave"]["thr_len"])


A_LEN = {"A": 30, "B": 8, "C": 12}
CASES = {
    "reference": _reference,
    # A (block 1) in three intervals; its nodes on path 1: forward at position 0, reverse at position 2
    "three_intervals_both_strands": lambda: synth(tg.graph([(False, "A+ B+ A-")], lens=A_LEN), {1: pieces(3, 10, 500)}),
    # members 0 .. 3 of A are dropped from every interval: positions 0, 2 and 4 of path 1, and all of path 2; member 4 (path 3) stays
    "dropped_everywhere": lambda: synth(tg.graph([(False, "A+ B+ A+ B+ A+"), (False, "A+"), (True, "B+ A+")], lens=A_LEN), {1: pieces(2, 15, 500)}, drop=lambda b, m, j: m < 4),
    "two_nodes_one_block": lambda: synth(tg.graph([(True, "A+ A- B+")], lens=A_LEN), {1: pieces(2, 15, 500)}),
    "circular_ends": lambda: synth(tg.graph([(True, "A+ B+ C+ A-")], lens=A_LEN), {1: pieces(3, 10, 500)}),
    "tile_1023": lambda: tile_case(TILE - 1),
    "tile_1024": lambda: tile_case(TILE),
    "tile_1025": lambda: tile_case(TILE + 1),
    "second_level": second_level_case,
    "forty_intervals": lambda: synth(tg.graph([(False, "A+ B+ A-"), (True, "A-")], lens={"A": 400, "B": 8}), {1: pieces(40, 10, 600)}),
    # survivors 100 and 200; new ids below, between and above them, two of them at or above 2^63
    "id_ranges": lambda: synth(tg.graph([(False, "A+ B+ C+"), (True, "C- A-")], lens={"A": 50, "B": 8, "C": 9}, ids={"A": 120, "B": 100, "C": 200}),
                               {120: [(0, 10, (1 << 64) - 1, False, False), (10, 20, 150, False, False), (20, 30, 50, False, False), (30, 40, 1 << 63, False, False),
                                      (40, 50, 199, False, False)]}),
    # A and B of depth 4 each, merged into block 900 (A the anchor), each with an unaligned rest
    "interleaved_merge": lambda: synth(tg.graph([(False, "A+ B+"), (False, "B- A-"), (True, "A+ C+ B+"), (True, "B+ A-")], lens={"A": 30, "B": 25, "C": 5}),
                                       {1: [(0, 20, 900, True, True), (20, 30, 901, False, False)], 2: [(0, 5, 902, False, False), (5, 25, 900, True, False)]}),
    "high_index": lambda: synth(tg.graph([(False, "A+ B+ A-")], lens=A_LEN), {1: pieces(3, 10, 500)}, shift=(1 << 16) + 5),
    # the middle slice keeps nobody: its block is listed with depth 0
    "empty_unaligned": lambda: synth(tg.graph([(False, "A+ B+ A-")], lens=A_LEN), {1: pieces(3, 10, 500)}, drop=lambda b, m, j: j == 1),
    "no_cut": lambda: synth(tg.graph([(False, "A+ B+ A-")], lens=A_LEN), {}),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ---------------------------------------------------------------- seeded random graphs over the levels of reweave_gen
def random_graph(seed):
    """the blocks of the first group of reweave_gen.random_level(seed) that reweave accepts, and up to three blocks without a hit, laid on
    random paths: both strands, circular and linear, every member of a block on some path -> (g, matches)"""
    rng = random.Random(77000 + seed)
    groups, all_matches = rg.random_level(seed)
    blks = groups[0]
    matches = [dict(m, qry=blks[m["qry"]]["block_id"], ref=blks[m["ref"]]["block_id"]) for m in all_matches if m["group"] == 0]
    blks = blks + [{"block_id": rng.randrange(1 << 64), "depth": rng.randint(1, 3), "consensus": rg.letters(rng, rng.randint(1, 30))} for _ in range(rng.randint(0, 3))]
    n_paths = rng.randint(1, 4)
    walk = [[] for _ in range(n_paths)]
    for b in blks:
        for _ in range(b["depth"]):
            walk[rng.randrange(n_paths)].append(b)
    g = {"paths": {}, "nodes": {}, "blocks": {b["block_id"]: {"consensus": b["consensus"], "alignments": {}} for b in blks}}
    ids = iter(rng.sample(range(1, 1 << 62), sum(b["depth"] for b in blks)))
    for k, w in enumerate(walk):
        rng.shuffle(w)
        tot = sum(len(b["consensus"]) for b in w) + rng.randint(1, 50)
        path = g["paths"][3 * k + 1] = {"nodes": [], "tot_len": tot, "circular": rng.random() < 0.5, "name": None}
        at = rng.randrange(tot) if path["circular"] else 0
        for b in w:
            nid, ln = next(ids), len(b["consensus"])
            end = (at + ln) % tot if path["circular"] else at + ln
            g["nodes"][nid] = {"block_id": b["block_id"], "path_id": 3 * k + 1, "strand": rng.choice("+-"), "position": (at, end)}
            g["blocks"][b["block_id"]]["alignments"][nid] = {"subs": [], "dels": [], "inss": []}
            path["nodes"].append(nid)
            at = end
    return g, matches


@functools.lru_cache(maxsize=None)
def random_case(seed):
    g, matches = random_graph(seed)
    return host_apply(g, matches, rr.expected_call, ref_slicer)


def simplify_cases():
    """the cases whose graph after goes on to pga_plan_simplify: pieces of one block that follow each other on every path are transitive edges"""
    return [case(n) for n in ("reference", "forty_intervals", "circular_ends", "id_ranges", "tile_1024", "three_intervals_both_strands", "interleaved_merge")] + \
        [random_case(seed) for seed in range(16)]


def fresh_cut(c, seed=0):
    """a second round behind case c: up to three of the blocks the first call made (depth >= 1), each cut into two unaligned intervals ->
    the case whose graph is c's graph after, or None"""
    rng = random.Random(500 + seed)
    after = c["after"]
    made = [b for b in (after["blocks"]) if b not in c["before"]["blocks"] and after["blocks"][b]["alignments"] and len(after["blocks"][b]["consensus"]) >= 2]
    if not made:
        return None
    lists = tg.to_lists(after, {b: sorted(blk["alignments"]) for b, blk in after["blocks"].items()})
    cuts = {}
    for b in rng.sample(sorted(made), min(3, len(made))):
        ln = len(after["blocks"][b]["consensus"])
        cuts[b] = [(0, ln // 2, rng.randrange(1 << 64), False, False), (ln // 2, ln, rng.randrange(1 << 64), False, False)]
    nxt = synth_graph(after, cuts)
    assert nxt["args"][:3] == lists
    return nxt

