"""`pangraph simplify` restated for the tests, function by function: commands/simplify/simplify_run.rs:23-38, Pangraph::remove_path
(pangraph/pangraph.rs:110-132), circularize/circularize.rs:11-76, circularize/circularize_utils.rs (SimpleNode, Edge), circularize/
merge_blocks.rs:15-234, PangraphBlock::reverse_complement (pangraph_block.rs:63-75), Edit::{reverse_complement, shift, concat}
(edits.rs:257-304, per item edits.rs:29-41, 68-80, 99-111) and PangraphNode::new(None, ..)'s id.  Independent of pangraph_amd/simplify.py.

A graph is {"paths": {pid: {"nodes": [nid], "tot_len", "circular", "name"}}, "blocks": {bid: {"consensus": str, "alignments": {nid: edit}}},
"nodes": {nid: {"block_id", "path_id", "strand": "+" | "-", "position": (start, end)}}} with int keys (the reference's BTreeMaps: iteration
is in sorted key order) and edit = {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]} (Vecs: list order is compared).
An edge is ((bid, strand), (bid, strand)).

remove_transitive_edges takes `first()` of a HashMap iteration, an undefined order; here the order is an explicit SCHEDULE, a list of rounds,
each a list of edges, applied one after the other with merge_blocks."""
import copy
import struct

COMPLEMENT = dict(zip("ACGTYRWSKMDVHBN-", "TGCARYWSMKHBDVN-"))      # io/seq.rs:9-29


class Rejected(Exception):
    """the reference returns Err: a letter the complement table does not hold"""


def from_json(g):
    """a parsed pangraph JSON -> the graph shape above (a deep copy)"""
    return {
        "paths": {int(k): {"nodes": [int(n) for n in p["nodes"]], "tot_len": p["tot_len"], "circular": bool(p["circular"]), "name": p.get("name")} for k, p in g["paths"].items()},
        "blocks": {int(k): {"consensus": b["consensus"], "alignments": {int(n): {"subs": [(x["pos"], x["alt"]) for x in e["subs"]], "dels": [(x["pos"], x["len"]) for x in e["dels"]],
                                                                                 "inss": [(x["pos"], x["seq"]) for x in e["inss"]]} for n, e in b["alignments"].items()}} for k, b in g["blocks"].items()},
        "nodes": {int(k): {"block_id": int(n["block_id"]), "path_id": int(n["path_id"]), "strand": n["strand"], "position": tuple(n["position"])} for k, n in g["nodes"].items()},
    }


# ---------------------------------------------------------------- PangraphNode::new(None, ..): XXH64, seed 0, of five little-endian u64 words
_M = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = 11400714785074694791, 14029467366897019727, 1609587929392839161, 9650029242287828579, 2870177450012600261


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & _M


def _round(acc, lane):
    return (_rotl((acc + lane * _P2) & _M, 31) * _P1) & _M


def _merge_round(h, v):
    return ((h ^ _round(0, v)) * _P1 + _P4) & _M


def xxh64(data, seed=0):
    n, i = len(data), 0
    if n >= 32:
        v = [(seed + _P1 + _P2) & _M, (seed + _P2) & _M, seed, (seed - _P1) & _M]
        while i + 32 <= n:
            for k in range(4):
                v[k] = _round(v[k], struct.unpack_from("<Q", data, i + 8 * k)[0])
            i += 32
        h = (_rotl(v[0], 1) + _rotl(v[1], 7) + _rotl(v[2], 12) + _rotl(v[3], 18)) & _M
        for k in range(4):
            h = _merge_round(h, v[k])
    else:
        h = (seed + _P5) & _M
    h = (h + n) & _M
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, i)[0]), 27) * _P1 + _P4) & _M
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, i)[0] * _P1 & _M), 23) * _P2 + _P3) & _M
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * _P5 & _M), 11) * _P1) & _M
        i += 1
    h ^= h >> 33
    h = (h * _P2) & _M
    h ^= h >> 29
    h = (h * _P3) & _M
    return h ^ (h >> 32)


def node_id(block_id, path_id, strand, position):
    return xxh64(struct.pack("<5Q", block_id, path_id, 0 if strand == "+" else 1, position[0], position[1]))


def new_node(block_id, path_id, strand, position):
    return {"id": node_id(block_id, path_id, strand, position), "block_id": block_id, "path_id": path_id, "strand": strand, "position": tuple(position)}


# ---------------------------------------------------------------- edits.rs
def complement(c):
    if c not in COMPLEMENT:
        raise Rejected(f"Unknown nucleotide character: '{c}'")
    return COMPLEMENT[c]


def reverse_complement(seq):
    return "".join(complement(c) for c in reversed(seq))


def edit_reverse_complement(e, ln):
    """edits.rs:257-276: every list mapped, then sort_by_key(pos) -- a stable sort, as Python's"""
    subs = sorted([(ln - pos - 1, complement(alt)) for pos, alt in e["subs"]], key=lambda x: x[0])
    dels = sorted([(ln - pos - l, l) for pos, l in e["dels"]], key=lambda x: x[0])
    inss = sorted([(ln - pos, reverse_complement(seq)) for pos, seq in e["inss"]], key=lambda x: x[0])
    return {"subs": subs, "dels": dels, "inss": inss}


def edit_shift(e, shift):
    return {"inss": [(pos + shift, seq) for pos, seq in e["inss"]], "dels": [(pos + shift, l) for pos, l in e["dels"]], "subs": [(pos + shift, alt) for pos, alt in e["subs"]]}


def edit_concat(a, nxt):
    """edits.rs:286-304"""
    inss, dels, subs = list(a["inss"]), list(a["dels"]), list(a["subs"])
    for pos, seq in nxt["inss"]:
        for k, (p, s) in enumerate(inss):
            if p == pos:
                inss[k] = (p, s + seq)
                break
        else:
            inss.append((pos, seq))
    dels.extend(nxt["dels"])
    subs.extend(nxt["subs"])
    return {"subs": subs, "dels": dels, "inss": inss}


def block_reverse_complement(b):
    """pangraph_block.rs:63-75"""
    ln = len(b["consensus"])
    return {"consensus": reverse_complement(b["consensus"]), "alignments": {nid: edit_reverse_complement(e, ln) for nid, e in sorted(b["alignments"].items())}}


# ---------------------------------------------------------------- circularize_utils.rs
def flip(strand):
    return "-" if strand == "+" else "+"


def node_invert(n):
    return (n[0], flip(n[1]))


def edge_invert(e):
    return (node_invert(e[1]), node_invert(e[0]))


def edge_eq(a, b):
    return a == b or a == edge_invert(b)


def conventional_orientation(e):
    n1, n2 = e
    return e if (n1[0] < n2[0]) or (n1[0] == n2[0] and n1[1] == "+") else edge_invert(e)


def to_tuple(e):
    return (e[0][0], e[1][0], 0 if e[0][1] == "+" else 1, 0 if e[1][1] == "+" else 1)


def path_edges(g, path):
    sn = [(g["nodes"][n]["block_id"], g["nodes"][n]["strand"]) for n in path["nodes"]]
    edges = list(zip(sn, sn[1:]))
    if path["circular"]:
        edges.append((sn[-1], sn[0]))
    return edges


# ---------------------------------------------------------------- circularize.rs
def count_edges(g):
    """a list of [edge, count] under Edge's equality (the HashMap keeps the key it saw first)"""
    table = {}
    for _, path in sorted(g["paths"].items()):
        for e in path_edges(g, path):
            key = min(e, edge_invert(e))
            table.setdefault(key, [e, 0])[1] += 1
    return list(table.values())


def find_transitive_edges(g):
    depth = {bid: len(b["alignments"]) for bid, b in g["blocks"].items()}
    out = [e for e, n in count_edges(g) if depth[e[0][0]] == n and depth[e[1][0]] == n and e[0][0] != e[1][0]]
    return sorted(out, key=lambda e: to_tuple(conventional_orientation(e)))


# ---------------------------------------------------------------- pangraph.rs:110-132
def remove_path(g, pid):
    path = g["paths"].pop(pid, None)
    if path is not None:
        for nid in path["nodes"]:
            node = g["nodes"].pop(nid, None)
            if node is not None and node["block_id"] in g["blocks"]:
                g["blocks"][node["block_id"]]["alignments"].pop(nid, None)
    for bid in [bid for bid, b in g["blocks"].items() if not b["alignments"]]:
        del g["blocks"][bid]


# ---------------------------------------------------------------- merge_blocks.rs
def orient_merging_edge(g, e):
    l1, l2 = len(g["blocks"][e[0][0]]["consensus"]), len(g["blocks"][e[1][0]]["consensus"])
    return e if l1 > l2 or (l1 == l2 and e[0][0] < e[1][0]) else edge_invert(e)


def find_node_pairings(g, edge):
    pairings, new_nodes = {}, {}
    for path_id, path in sorted(g["paths"].items()):
        n = len(path["nodes"])
        for idx in range(n if path["circular"] else n - 1):
            nid1, nid2 = path["nodes"][idx], path["nodes"][(idx + 1) % n]
            n1, n2 = g["nodes"][nid1], g["nodes"][nid2]
            sn1, sn2 = (n1["block_id"], n1["strand"]), (n2["block_id"], n2["strand"])
            if edge_eq(edge, (sn1, sn2)):
                pairings[nid1] = nid2
                pairings[nid2] = nid1
                new_strand = n1["strand"] if edge[0] == sn1 else n2["strand"]
                node = new_node(edge[0][0], path_id, new_strand, (n1["position"][0], n2["position"][1]))
                new_nodes[nid1] = node
                new_nodes[nid2] = dict(node)
    return pairings, new_nodes


def concatenate_alignments(bl1, bl2, node_map, new_node_ids):
    aln = {}
    for nid1, e1 in sorted(bl1["alignments"].items()):
        e2 = bl2["alignments"][node_map[nid1]]
        aln[new_node_ids[nid1]] = edit_concat(e1, edit_shift(e2, len(bl1["consensus"])))
    return {"consensus": bl1["consensus"] + bl2["consensus"], "alignments": aln}


def merge_alignment(g, edge, node_map, new_nodes):
    new_ids = {k: n["id"] for k, n in new_nodes.items()}
    b1 = g["blocks"][edge[0][0]]
    b2 = g["blocks"][edge[1][0]]
    if edge[0][1] != edge[1][1]:
        b2 = block_reverse_complement(b2)
    b_left, b_right = (b1, b2) if edge[0][1] == "+" else (b2, b1)
    return concatenate_alignments(b_left, b_right, node_map, new_ids)


def graph_merging_update_paths(g, new_nodes, bid_left):
    for path in g["paths"].values():
        kept = []
        for nid in path["nodes"]:
            if nid in new_nodes:
                if g["nodes"][nid]["block_id"] == bid_left:
                    kept.append(new_nodes[nid]["id"])
            else:
                kept.append(nid)
        path["nodes"] = kept


def graph_merging_update_nodes(g, new_nodes, bid_left):
    for nid, n in sorted(new_nodes.items()):
        if g["nodes"][nid]["block_id"] == bid_left:
            g["nodes"][n["id"]] = {k: v for k, v in n.items() if k != "id"}
        del g["nodes"][nid]


def merge_blocks(g, edge):
    edge = orient_merging_edge(g, edge)
    node_map, new_nodes = find_node_pairings(g, edge)
    new_block = merge_alignment(g, edge, node_map, new_nodes)
    del g["blocks"][edge[0][0]]
    del g["blocks"][edge[1][0]]
    g["blocks"][edge[0][0]] = new_block
    graph_merging_update_paths(g, new_nodes, edge[0][0])
    graph_merging_update_nodes(g, new_nodes, edge[0][0])


def remove_transitive_edges(g, schedule):
    """the schedule's edges one after the other; every one must be transitive when its turn comes, and none may be left at the end"""
    for rnd in schedule:
        for e in rnd:
            assert any(edge_eq(e, t) for t in find_transitive_edges(g)), f"the schedule names an edge that is not transitive: {e}"
            merge_blocks(g, e)
    assert not find_transitive_edges(g), "the schedule leaves transitive edges"


def simplify(g, focal_names, schedule):
    """simplify_run.rs:23-38 on a copy"""
    g = copy.deepcopy(g)
    for pid in [pid for pid, p in sorted(g["paths"].items()) if p["name"] not in focal_names]:
        remove_path(g, pid)
    remove_transitive_edges(g, schedule)
    return g


# ---------------------------------------------------------------- one concatenation in the shape pangraph_amd.simplify.merge_blocks takes
def merge_batch(blocks, edges):
    """blocks: [{"consensus", "members": [edit]}]; edges: [{"left", "right", "left_rc", "right_rc", "partner"}] -> per edge {"status",
    "consensus", "members"}; status 2: the reference's Err (consensus and members None)"""
    out = []
    for e in edges:
        try:
            side = []
            for b, rc in ((blocks[e["left"]], e["left_rc"]), (blocks[e["right"]], e["right_rc"])):
                blk = {"consensus": b["consensus"], "alignments": dict(enumerate(b["members"]))}
                side.append(block_reverse_complement(blk) if rc else blk)
            node_map = dict(enumerate(e["partner"]))
            new = concatenate_alignments(side[0], side[1], node_map, {k: k for k in node_map})
            out.append({"status": 0, "consensus": new["consensus"], "members": [new["alignments"][k] for k in sorted(new["alignments"])]})
        except Rejected:
            out.append({"status": 2, "consensus": None, "members": None})
    return out


def merged_counts(blocks, e):
    """what does not depend on a status: per output member (n_subs, n_dels, n_inss) -- positions alone decide the insertions"""
    masked = [{"consensus": "A" * len(b["consensus"]), "members": [{"subs": [(p, "A") for p, _ in m["subs"]], "dels": list(m["dels"]), "inss": [(p, "A" * len(s)) for p, s in m["inss"]]}
                                                                    for m in b["members"]]} for b in blocks]
    r = merge_batch(masked, [e])[0]
    return [(len(m["subs"]), len(m["dels"]), len(m["inss"])) for m in r["members"]], [[len(s) for _, s in m["inss"]] for m in r["members"]]
