"""Graphs for pga_plan_simplify (pangraph_amd/topology.py) and the expectation they are held against: `host_plan`, one round of the path
side built from the host functions of pangraph_amd/simplify.py (find_transitive_edges, choose_round, orient_merging_edge,
find_node_pairings, graph_merging_update) on the lists the device call takes.  Every graph is built so that the structure a test aims at
exists by construction; tests/test_topo_cpu.py pins each of them on the host functions, so a generator that stops producing its case
fails there and not silently on the GPU.

A graph here is (blocks, paths, nodes) as topology.pack_lists takes them: blocks [(block_id, cons_len, depth, alive)], paths [(path_id,
node_off, n_nodes, circular)], nodes [(node_id, pos0, pos1, block index, member, reverse)]."""
import random

from pangraph_amd import simplify as sp
from pangraph_amd import topology as tp

TILE = tp.TILE
PAIR_GROUP = 256                         # threads per workgroup of the pairing kernel (TP_THREADS of pga_topo_idx.h)
EDIT = {"subs": [], "dels": [], "inss": []}
STRAND = "+-"


# ---------------------------------------------------------------- lists <-> the dict shape of simplify.normalize
def to_graph(blocks, paths, nodes):
    """-> (g, order, bids): the dict graph of the alive blocks (consensus 'A' * cons_len), the member order, the id of every block index"""
    bids = [b[0] for b in blocks]
    g = {"paths": {}, "nodes": {}, "blocks": {b[0]: {"consensus": "A" * b[1], "alignments": {}} for b in blocks if b[3]}}
    order = {b[0]: [None] * b[2] for b in blocks if b[3]}
    for pid, off, n, circular in paths:
        g["paths"][pid] = {"nodes": [x[0] for x in nodes[off:off + n]], "tot_len": 0, "circular": bool(circular), "name": None}
        for nid, pos0, pos1, b, member, rev in nodes[off:off + n]:
            g["nodes"][nid] = {"block_id": bids[b], "path_id": pid, "strand": STRAND[1 if rev else 0], "position": (pos0, pos1)}
            g["blocks"][bids[b]]["alignments"][nid] = EDIT
            order[bids[b]][member] = nid
    return g, order, bids


def to_lists(g, order):
    return tp.unpack_lists(tp.pack_graph(g, order))


def count_edges(g):
    """every edge with its count, conventional orientation, sorted as the transitive list is (count_edges of circularize.rs)"""
    count = {}
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        sn = [(g["nodes"][n]["block_id"], g["nodes"][n]["strand"]) for n in p["nodes"]]
        for e in list(zip(sn, sn[1:])) + ([(sn[-1], sn[0])] if p["circular"] and sn else []):
            c = sp._conventional(e)
            count[c] = count.get(c, 0) + 1
    return sorted(count.items(), key=lambda kv: sp._sort_key(kv[0]))


def host_plan(blocks, paths, nodes, sched=None, flags=0):
    """what PlanOut.to_lists() gives for one round, from the host functions of simplify.py"""
    g, order, bids = to_graph(blocks, paths, nodes)
    index = {b: i for i, b in enumerate(bids) if blocks[i][3]}
    flat = lambda e, n: (index[e[0][0]], index[e[1][0]], STRAND.index(e[0][1]), STRAND.index(e[1][1]), n)
    transitive = sp.find_transitive_edges(g)
    res = {"transitive": [flat(e, len(order[e[0][0]])) for e in transitive], "edge_counts": [flat(e, n) for e, n in count_edges(g)] if flags & tp.COUNTS else [],
           "round": [], "partner": [], "new_nodes": [], "old_left": [], "old_right": [], "blocks": None, "paths": None, "nodes": None}
    if flags & tp.EDGES_ONLY:
        return res
    if sched is not None:
        rnd = [((bids[b1], STRAND[1 if s1 else 0]), (bids[b2], STRAND[1 if s2 else 0])) for b1, s1, b2, s2 in sched]
        assert rnd and all(sp._conventional(e) in transitive for e in rnd) and len({b for e in rnd for b in (e[0][0], e[1][0])}) == 2 * len(rnd)
    else:
        rnd = sp.choose_round(transitive)
    plans = []
    for e in rnd:
        o = sp.orient_merging_edge(g, e)
        pair, new = sp.find_node_pairings(g, o)
        (a, sa), (b, sb) = o
        rc = int(sa != sb)
        left, right, left_rc, right_rc = (a, b, 0, rc) if sa == "+" else (b, a, rc, 0)
        at = {n: i for i, n in enumerate(order[right])}
        res["round"].append({"anchor": index[a], "other": index[b], "anchor_rev": STRAND.index(sa), "other_rev": STRAND.index(sb), "transitive": transitive.index(sp._conventional(e)),
                             "merge": (index[left], index[right], left_rc, right_rc), "partner_off": len(res["partner"])})
        for k, n in enumerate(order[left]):
            nid, node = new[n]
            res["partner"].append(at[pair[n]])
            res["new_nodes"].append((nid, node["position"][0], node["position"][1], index[a], k, int(node["strand"] == "-")))
            res["old_left"].append(n)
            res["old_right"].append(pair[n])
        plans.append((o, new, [new[n][0] for n in order[left]]))
    if not rnd:
        return res
    for o, new, ids in plans:
        (a, _), (b, _) = o
        merged = {"consensus": g["blocks"][a]["consensus"] + g["blocks"][b]["consensus"], "alignments": {n: EDIT for n in ids}}
        sp.graph_merging_update(g, o, merged, new)
        del order[b]
        order[a] = ids
    slot = {n: k for ids in order.values() for k, n in enumerate(ids)}
    res["blocks"] = [(bid, len(g["blocks"][bid]["consensus"]), len(order[bid]), 1) if bid in order and blocks[i][3] else (bid, 0, 0, 0) for i, bid in enumerate(bids)]
    res["paths"], res["nodes"] = [], []
    for pid, _, _, circular in paths:
        ids = g["paths"][pid]["nodes"]
        res["paths"].append((pid, len(res["nodes"]), len(ids), circular))
        for n in ids:
            x = g["nodes"][n]
            res["nodes"].append((n, x["position"][0], x["position"][1], index[x["block_id"]], slot[n], int(x["strand"] == "-")))
    return res


# ---------------------------------------------------------------- small graphs written out
def graph(paths, lens=None, ids=None):
    """paths: [(circular, "A+ B- ...")], blocks named by a word; lens / ids: {name: cons_len / block id} (default 10 + 3 * rank, 1 + rank by name).
    Node ids are 101, 102, ... in path order; the members of a block are ordered by node id; positions are running coordinates."""
    names = sorted({w[:-1] for _, s in paths for w in s.split()} | set(lens or {}) | set(ids or {}))
    bid = {n: (ids or {}).get(n, 1 + r) for r, n in enumerate(names)}
    ln = {n: (lens or {}).get(n, 10 + 3 * r) for r, n in enumerate(names)}
    g = {"paths": {}, "nodes": {}, "blocks": {bid[n]: {"consensus": "A" * ln[n], "alignments": {}} for n in names if any(n == w[:-1] for _, s in paths for w in s.split())}}
    nid = 100
    for k, (circular, s) in enumerate(paths):
        p = g["paths"][k + 1] = {"nodes": [], "tot_len": 0, "circular": bool(circular), "name": None}
        at = 7 * k
        for w in s.split():
            nid += 1
            g["nodes"][nid] = {"block_id": bid[w[:-1]], "path_id": k + 1, "strand": w[-1], "position": (at, at + ln[w[:-1]])}
            at += ln[w[:-1]] + 1                                   # (strictly growing: no two new nodes of a path share block, strand and position, hence an id)
            g["blocks"][bid[w[:-1]]]["alignments"][nid] = EDIT
            p["nodes"].append(nid)
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    return to_lists(g, order)


def shift_blocks(lists, by):
    """the same graph behind `by` dead block entries: every block index grows by `by`"""
    blocks, paths, nodes = lists
    return ([(0, 0, 0, 0)] * by + blocks, paths, [(n[0], n[1], n[2], n[3] + by, n[4], n[5]) for n in nodes])


def tile_graph():
    """paths of TILE - 1, TILE and TILE + 1 positions, one behind the other, filled with the nodes of one deep block F; transitive pairs X_i Y_i
    sit where a pair straddles the edge of a tile of the splice or of a workgroup of the pairing, and across the wrap of the circular one"""
    spots = {}                                                        # global position of a pair's first node -> strands

    def lay(n, start, circular, pairs):
        words = ["F+"] * n
        for at, (s1, s2) in pairs:
            k = len(spots)
            spots[start + at] = (s1, s2)
            words[at], words[(at + 1) % n] = f"X{k:02d}{s1}", f"Y{k:02d}{s2}"
        return (circular, " ".join(words))

    a = lay(TILE - 1, 0, False, [(PAIR_GROUP - 1, "++"), (2 * PAIR_GROUP - 2, "-+"), (TILE - 3, "+-")])
    b = lay(TILE, TILE - 1, True, [(0, "++"), (PAIR_GROUP, "--")])                          # positions (TILE - 1, TILE): over the first tile's edge
    c = lay(TILE + 1, 2 * TILE - 1, True, [(TILE - PAIR_GROUP, "++"), (TILE, "--")])        # the last one wraps: (3 TILE - 1, 2 TILE - 1)
    return graph([a, b, c], lens={"F": 5}), spots


CASES = {
    # a pair across the wrap of a circular path: A (the longer: the anchor) is last, B at position 0 is dropped; C is too deep to take part
    "wrap_dropped_at_0": lambda: graph([(True, "B+ C+ A+"), (False, "C+")], lens={"A": 30, "B": 10}),
    "wrap_anchor_at_0": lambda: graph([(True, "A+ C+ B+"), (False, "C+")], lens={"A": 30, "B": 10}),
    "two_node_circular": lambda: graph([(True, "A+ B+")]),
    "linear_ends": lambda: graph([(False, "B+ C+ A+"), (False, "C+ D+ E+")]),
    "empty_and_single": lambda: graph([(False, ""), (True, "S+"), (False, "T-"), (True, ""), (False, "A+ B-"), (False, "")]),
    "chain": lambda: graph([(False, "A+ B+ C+ D+")]),
    "equal_lengths": lambda: graph([(False, "A+ B+")], lens={"A": 12, "B": 12}, ids={"A": 900, "B": 40}),
    "one_sided_depth": lambda: graph([(False, "A+ B+"), (False, "B+")]),
    "four_strands": lambda: graph([p for k, (s1, s2) in enumerate(("++", "+-", "-+", "--")) for p in
                                   ((False, f"X{k}{s1} Y{k}{s2}"), (False, f"Y{k}{STRAND[s2 == '+']} X{k}{STRAND[s1 == '+']}"))]),
    "self_loop": lambda: graph([(True, "A+ A+"), (False, "D+ E+")]),
    "reverse_anchor": lambda: graph([(False, "A- B+"), (False, "B- A+")], lens={"A": 40, "B": 9}),
    "high_indices": lambda: shift_blocks(graph([(True, "A+ B- C+"), (False, "C+ A+ B-")]), (1 << 16) + 5),
    "tile_edges": lambda: tile_graph()[0],
    "all_but_one": lambda: graph([(False, "A+ B+"), (True, "C+ D- E+ C+")]),
}


# ---------------------------------------------------------------- seeded random graphs: super-blocks cut into transitive pieces
def random_graph(seed):
    """super-blocks laid on paths in both directions, some cut into 2-4 consecutive pieces on every path that carries them: the pieces are
    transitive by construction.  Strands are mixed, block ids and lengths are drawn so that both anchor rules come up."""
    rng = random.Random(seed)
    n_super = rng.randint(2, 7)
    free_ids = rng.sample(range(1, 400), 4 * n_super)
    supers, lens, ids = [], {}, {}
    for s in range(n_super):
        pieces = []
        for k in range(rng.choice((1, 1, 2, 2, 3, 4))):
            name = f"S{s}P{k}"
            lens[name] = rng.choice((0, 5, 8, 8, 8, 13, 40))
            ids[name] = free_ids.pop()
            pieces.append((name, rng.choice(STRAND)))
        supers.append(pieces)
    paths = []
    for _ in range(rng.randint(1, 5)):
        words = []
        for _ in range(rng.randint(0, 6)):
            pieces = supers[rng.randrange(n_super)]
            if rng.random() < 0.4:
                pieces = [(n, STRAND[s == "+"]) for n, s in reversed(pieces)]
            words += [n + s for n, s in pieces]
        paths.append((rng.random() < 0.5, " ".join(words)))
    if not any(s for _, s in paths):
        paths.append((True, "".join(n + s + " " for n, s in supers[0]).strip()))
    return graph(paths, lens=lens, ids=ids)


def second_round(lists):
    """the graph behind the first defined round (host functions), or None when that round is empty"""
    res = host_plan(*lists)
    return (res["blocks"], res["paths"], res["nodes"]) if res["round"] else None
