"""`pangraph simplify` (packages/pangraph/src/commands/simplify/simplify_run.rs:23-38): the paths that are not asked for are removed
(Pangraph::remove_path, pangraph/pangraph.rs:110-132) and transitive edges are merged until none is left (circularize/circularize.rs:11-76,
circularize/merge_blocks.rs:15-234).  The graph bookkeeping, O(nodes), is done here; the block concatenations -- consensus letters and edit
lists -- are `pga_merge_blocks` (include/pga_align.h), one call per ROUND of disjoint edges.  ctypes only; the HIP library does the work.
With simplify(topology="device") the graph bookkeeping of a round is one `pga_plan_simplify` call as well (topology.py); with
simplify(paths="device") the removal of the paths is one `pga_remove_paths` call (remove.py) whose arrays the first round reads by pointer.

The reference merges `find_transitive_edges(graph).first()` of a HashMap iteration until none is left: its order is undefined, and for chains
the orientation and the id of the final block depend on it.  The DEFINED order here: in every round the transitive edges are sorted by
Edge::conventional_orientation().to_tuple() and taken greedily while both of their blocks are still unused in the round.  Edges that share no
block do not see each other's merge, so a round is one of the orders the reference may take."""
import ctypes as C

from . import batch
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_block_t, rc_member_t
from .reconstruct import _Packed


class merge_edge_t(C.Structure):
    _fields_ = [("left", C.c_uint32), ("right", C.c_uint32), ("left_rc", C.c_int32), ("right_rc", C.c_int32)]


class merge_res_t(C.Structure):
    _fields_ = [("status", C.c_int32), ("pad", C.c_int32), ("member_off", C.c_uint64)]


class merge_out_t(C.Structure):
    _fields_ = [("edges", C.POINTER(merge_res_t)), ("blocks", C.POINTER(rc_block_t)), ("members", C.POINTER(rc_member_t)), ("subs", C.POINTER(sub_t)),
                ("dels", C.POINTER(del_t)), ("inss", C.POINTER(ins_t)), ("ins_seq", C.POINTER(C.c_char)), ("cons", C.POINTER(C.c_char))]


class SimplifyError(Exception):
    """the reference returns Err: a block that has to be reverse-complemented holds a letter the complement table rejects"""


def _bind(dll):
    dll.pga_merge_blocks.restype = C.c_int
    dll.pga_merge_blocks.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(merge_out_t)]
    dll.pga_merge_free.restype = None
    dll.pga_merge_free.argtypes = [C.POINTER(merge_out_t)]
    dll.pga_last_error.restype = C.c_char_p


class MergeOut:
    """the output of one call; `graph_args()` are the first seven arguments of the next pga_merge_blocks call or of pga_reconstruct:
    pointers into this output, nothing is copied.  Lives until free()."""

    def __init__(self, dll, out, n_edges, keep):
        self.dll, self.out, self.n_edges, self.keep = dll, out, n_edges, keep          # keep: the input buffers are not needed any more, the caller's may be
        self.n_members = [out.blocks[e].n_members for e in range(n_edges)]
        self.member_off = [out.edges[e].member_off for e in range(n_edges)]
        self.status = [out.edges[e].status for e in range(n_edges)]

    def graph_args(self):
        o = self.out
        cast = lambda p: C.cast(p, C.c_void_p)
        return (self.n_edges, cast(o.blocks), cast(o.members), cast(o.subs), cast(o.dels), cast(o.inss), cast(o.ins_seq))

    def counts(self):
        """per edge, per member: (n_subs, n_dels, n_inss)"""
        o = self.out
        return [[(o.members[m].n_subs, o.members[m].n_dels, o.members[m].n_inss) for m in range(self.member_off[e], self.member_off[e] + self.n_members[e])]
                for e in range(self.n_edges)]

    def to_dicts(self, with_offsets=False):
        """per edge {"status", "consensus", "members": [edit]} (the letters of a status-2 edge are as built, not to be used)"""
        o = self.out
        res, s, d, i = [], 0, 0, 0
        ins_base = C.addressof(o.ins_seq.contents) if o.ins_seq else 0
        for e in range(self.n_edges):
            b = o.blocks[e]
            cons_at = C.c_void_p.from_address(C.addressof(b)).value                  # (the field is a c_char_p: reading it would stop at a NUL)
            cons = C.string_at(cons_at, b.cons_len).decode("latin-1") if b.cons_len else ""
            members = []
            for m in range(self.member_off[e], self.member_off[e] + b.n_members):
                c = o.members[m]
                ed = {"subs": [(o.subs[k].pos, chr(o.subs[k].alt & 255)) for k in range(s, s + c.n_subs)], "dels": [(o.dels[k].pos, o.dels[k].len) for k in range(d, d + c.n_dels)],
                      "inss": [(o.inss[k].pos, C.string_at(ins_base + o.inss[k].seq_off, o.inss[k].len).decode("latin-1")) for k in range(i, i + c.n_inss)]}
                if with_offsets:
                    ed["seq_off"] = [o.inss[k].seq_off for k in range(i, i + c.n_inss)]
                s += c.n_subs; d += c.n_dels; i += c.n_inss
                members.append(ed)
            res.append({"status": self.status[e], "consensus": cons, "members": members})
            if with_offsets:
                res[-1]["cons_off"] = cons_at - C.addressof(o.cons.contents)
        return res

    def free(self):
        if self.out is not None:
            self.dll.pga_merge_free(C.byref(self.out))
            self.out = None


def merge_blocks_raw(graph_args, edges, partner, dll=None, keep=None):
    """graph_args: (n_blocks, blocks, members, subs, dels, inss, ins_seq) as C arrays or pointers (a _Packed's args()[:7], or a MergeOut's
    graph_args()); edges: [(left, right, left_rc, right_rc)]; partner: the concatenated partner lists -> MergeOut"""
    dll = dll or batch.lib()
    _bind(dll)
    E = (merge_edge_t * max(len(edges), 1))(*[merge_edge_t(l, r, 1 if lrc else 0, 1 if rrc else 0) for l, r, lrc, rrc in edges])
    P = (C.c_uint32 * max(len(partner), 1))(*partner)
    out = merge_out_t()
    if dll.pga_merge_blocks(*graph_args, len(edges), E, P if partner is not None else None, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return MergeOut(dll, out, len(edges), keep)


def merge_blocks(blocks, edges, dll=None):
    """blocks: [{"consensus": str, "members": [edit]}] with edit = {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]};
    edges: [{"left", "right", "left_rc", "right_rc", "partner": [index in the right block of the member joined with left member k]}]
    -> per edge {"status", "consensus", "members": [edit] in the left block's member order}"""
    K = _Packed(blocks, [])
    partner = [q for e in edges for q in e["partner"]]
    out = merge_blocks_raw(K.args()[:7], [(e["left"], e["right"], e["left_rc"], e["right_rc"]) for e in edges], partner, dll, keep=K)
    try:
        return out.to_dicts()
    finally:
        out.free()


# ---------------------------------------------------------------- PangraphNode::new(None, ..): XXH64 (seed 0) of five little-endian u64 words
_MASK = 0xFFFFFFFFFFFFFFFF
_PRIME = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5)


def _rol(x, r):
    return ((x << r) & _MASK) | (x >> (64 - r))


def _xxh64_40(words):
    """XXH64 with seed 0 of exactly five u64 words (40 bytes: one 32-byte stripe and one 8-byte tail)"""
    p1, p2, p3, p4, _ = _PRIME
    acc = [(p1 + p2) & _MASK, p2, 0, (-p1) & _MASK]
    acc = [(_rol((a + w * p2) & _MASK, 31) * p1) & _MASK for a, w in zip(acc, words[:4])]
    h = (_rol(acc[0], 1) + _rol(acc[1], 7) + _rol(acc[2], 12) + _rol(acc[3], 18)) & _MASK
    for a in acc:
        h = ((h ^ ((_rol((a * p2) & _MASK, 31) * p1) & _MASK)) * p1 + p4) & _MASK
    h = (h + 40) & _MASK
    k = (_rol((words[4] * p2) & _MASK, 31) * p1) & _MASK
    h = (_rol(h ^ k, 27) * p1 + p4) & _MASK
    h ^= h >> 33
    h = (h * p2) & _MASK
    h ^= h >> 29
    h = (h * p3) & _MASK
    return h ^ (h >> 32)


def node_id(block, path, reverse, position):
    """the id PangraphNode::new(None, block, path, strand, position) gives itself"""
    return _xxh64_40([block & _MASK, path & _MASK, 1 if reverse else 0, position[0] & _MASK, position[1] & _MASK])


# ---------------------------------------------------------------- the graph level: host bookkeeping, O(nodes)
def normalize(g):
    """a parsed pangraph JSON (or a graph already in this shape) -> {"paths": {pid: {"nodes", "tot_len", "circular", "name"}}, "blocks": {bid:
    {"consensus", "alignments": {nid: edit}}}, "nodes": {nid: {"block_id", "path_id", "strand", "position"}}}, int keys, a copy"""
    def edit(e):
        get = lambda x, a, b: (x[a], x[b]) if isinstance(x, dict) else (x[0], x[1])
        return {"subs": [get(x, "pos", "alt") for x in e["subs"]], "dels": [get(x, "pos", "len") for x in e["dels"]], "inss": [get(x, "pos", "seq") for x in e["inss"]]}
    return {"paths": {int(k): {"nodes": [int(n) for n in p["nodes"]], "tot_len": p["tot_len"], "circular": bool(p["circular"]), "name": p.get("name")} for k, p in g["paths"].items()},
            "blocks": {int(k): {"consensus": b["consensus"], "alignments": {int(n): edit(e) for n, e in b["alignments"].items()}} for k, b in g["blocks"].items()},
            "nodes": {int(k): {"block_id": int(n["block_id"]), "path_id": int(n["path_id"]), "strand": n["strand"], "position": tuple(n["position"])} for k, n in g["nodes"].items()}}


def remove_path(g, pid):
    path = g["paths"].pop(pid, None)
    for nid in (path["nodes"] if path else []):
        node = g["nodes"].pop(nid, None)
        if node and node["block_id"] in g["blocks"]:
            g["blocks"][node["block_id"]]["alignments"].pop(nid, None)
    for bid in [b for b, blk in g["blocks"].items() if not blk["alignments"]]:
        del g["blocks"][bid]


def _inv(e):
    (b1, s1), (b2, s2) = e
    return ((b2, "+" if s2 == "-" else "-"), (b1, "+" if s1 == "-" else "-"))


def _conventional(e):
    (b1, s1), (b2, _) = e
    return e if b1 < b2 or (b1 == b2 and s1 == "+") else _inv(e)


def _sort_key(e):
    (b1, s1), (b2, s2) = _conventional(e)
    return (b1, b2, int(s1 == "-"), int(s2 == "-"))


def find_transitive_edges(g):
    """edges between two different blocks that every node of both blocks lies on, sorted by conventional_orientation().to_tuple()"""
    count = {}
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        sn = [(g["nodes"][n]["block_id"], g["nodes"][n]["strand"]) for n in p["nodes"]]
        pairs = list(zip(sn, sn[1:])) + ([(sn[-1], sn[0])] if p["circular"] and sn else [])
        for e in pairs:
            c = _conventional(e)
            count[c] = count.get(c, 0) + 1
    depth = {b: len(blk["alignments"]) for b, blk in g["blocks"].items()}
    return sorted((e for e, n in count.items() if e[0][0] != e[1][0] and depth[e[0][0]] == n and depth[e[1][0]] == n), key=_sort_key)


def orient_merging_edge(g, e):
    """the anchor first: the longer consensus, on a tie the numerically smaller block id"""
    l1, l2 = len(g["blocks"][e[0][0]]["consensus"]), len(g["blocks"][e[1][0]]["consensus"])
    return e if (l1, -e[0][0]) > (l2, -e[1][0]) else _inv(e)


def find_node_pairings(g, edge):
    """-> (pairings {nid: nid}, new_nodes {old nid: (new id, node)}); the new node keeps (n1.position.0, n2.position.1) in path order and
    the strand of the anchor block's node"""
    pair, new = {}, {}
    inv = _inv(edge)
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        n = len(p["nodes"])
        for i in range(n if p["circular"] else n - 1):
            a, b = p["nodes"][i], p["nodes"][(i + 1) % n]
            na, nb = g["nodes"][a], g["nodes"][b]
            here = ((na["block_id"], na["strand"]), (nb["block_id"], nb["strand"]))
            if here == edge or here == inv:
                pair[a], pair[b] = b, a
                strand = na["strand"] if here[0] == edge[0] else nb["strand"]
                pos = (na["position"][0], nb["position"][1])
                nid = node_id(edge[0][0], pid, strand == "-", pos)
                new[a] = new[b] = (nid, {"block_id": edge[0][0], "path_id": pid, "strand": strand, "position": pos})
    return pair, new


def graph_merging_update(g, edge, new_block, new):
    """graph_merging_update_paths / _nodes and the block maps"""
    anchor = edge[0][0]
    del g["blocks"][edge[0][0]], g["blocks"][edge[1][0]]
    g["blocks"][anchor] = new_block
    for p in g["paths"].values():
        p["nodes"] = [new[n][0] if n in new else n for n in p["nodes"] if n not in new or g["nodes"][n]["block_id"] == anchor]
    for old in sorted(new):
        if g["nodes"][old]["block_id"] == anchor:
            g["nodes"][new[old][0]] = dict(new[old][1])
        del g["nodes"][old]


def choose_round(transitive):
    """greedily, in the sorted order, the edges whose two blocks are still unused"""
    used, rnd = set(), []
    for e in transitive:
        if e[0][0] not in used and e[1][0] not in used:
            rnd.append(e)
            used |= {e[0][0], e[1][0]}
    return rnd


class _DeviceRounds:
    """one pga_merge_blocks call per round.  A round whose blocks all lie in the previous round's output passes that output's arrays on
    as they are (pointers only); otherwise the blocks the round names are packed from the graph.  `prev` / `prev_at` stand for a round
    before the first: an object with graph_args() (the seven block arguments) and free(), and the index of every block id in its arrays
    (remove.Removed: the output of pga_remove_paths)."""

    def __init__(self, dll, prev=None, prev_at=None):
        self.dll, self.prev, self.prev_at, self.zero_copy = dll, prev, dict(prev_at or {}), []

    def __call__(self, g, order, jobs):
        named = []
        for j in jobs:
            named += [j["left"], j["right"]]
        if self.prev is not None and all(b in self.prev_at for b in named):
            at, args, keep = self.prev_at, self.prev.graph_args(), self.prev
            self.zero_copy.append(True)
        else:
            at = {b: i for i, b in enumerate(named)}
            K = _Packed([{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in named], [])
            args, keep = K.args()[:7], K
            self.zero_copy.append(False)
        out = merge_blocks_raw(args, [(at[j["left"]], at[j["right"]], j["left_rc"], j["right_rc"]) for j in jobs], [q for j in jobs for q in j["partner"]], self.dll, keep=keep)
        if self.prev is not None:
            self.prev.free()
        self.prev, self.prev_at = out, {j["anchor"]: i for i, j in enumerate(jobs)}
        return out.to_dicts()

    def close(self):
        if self.prev is not None:
            self.prev.free()
            self.prev = None


def _simplify_planned(g, order, dll, schedule, merge, trace, topology, first=None):
    """simplify()'s loop with the path side in pga_plan_simplify (topology.py): the graph is packed once, every round is one call whose
    output arrays are the next round's input, `round` and `partner` feed the block merge as they come, and the dicts are rebuilt once at
    the end.  Inside the loop only blocks are touched on the host: O(merged members), no walk over paths or nodes.
    first (a remove.Removed): the graph is not packed at all -- the planner starts on the arrays pga_remove_paths left, whose block indices
    are those of the loaded graph (first.bids), dead blocks included."""
    from . import topology as tp
    args = tp.pack_graph(g, order) if first is None else first.args
    planner = tp.DevicePlanner(args, dll) if topology == "device" else tp.StandInPlanner(args, topology)
    bids = sorted(g["blocks"]) if first is None else first.bids
    index = {b: i for i, b in enumerate(bids)}
    strand = lambda rev: "-" if rev else "+"
    blocks = {"blocks": {b: {"consensus": g["blocks"][b]["consensus"], "alignments": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in sorted(g["blocks"])}}
    slots = {b: range(len(order[b])) for b in blocks["blocks"]}                   # (a block's members are named by their slot from here on)
    device, rounds, lists = None, [], []
    try:
        while True:
            sched = None
            if schedule is not None and len(rounds) < len(schedule):
                if not planner.step(flags=tp.EDGES_ONLY)["transitive"]:
                    break
                given = [tuple(map(tuple, e)) for e in schedule[len(rounds)]]
                if not given or any(b not in index or b not in blocks["blocks"] for e in given for b in (e[0][0], e[1][0])):
                    raise ValueError("a round of the schedule is empty or names a block that does not exist")
                sched = [(index[b1], s1 == "-", index[b2], s2 == "-") for (b1, s1), (b2, s2) in given]
            try:
                res = planner.step(sched)
            except batch.PgaError as err:
                if sched is None:
                    raise
                raise ValueError(f"a round of the schedule names an edge that is not transitive, or uses a block twice ({err})")
            transitive =[((bids[b1], strand(s1)), (bids[b2], strand(s2))) for b1, b2, s1, s2, _ in res["transitive"]]
            if not transitive:
                break
            lists.append(transitive)
            jobs = []
            for r in res["round"]:
                left, right, left_rc, right_rc = r["merge"]
                jobs.append({"left": bids[left], "right": bids[right], "left_rc": bool(left_rc), "right_rc": bool(right_rc), "anchor": bids[r["anchor"]], "other": bids[r["other"]],
                             "partner": list(res["partner"][r["partner_off"]:r["partner_off"] + len(slots[bids[left]])])})
            if merge is not None:
                named = [b for j in jobs for b in (j["left"], j["right"])]
                at = {b: i for i, b in enumerate(named)}
                out = merge([{"consensus": blocks["blocks"][b]["consensus"], "members": blocks["blocks"][b]["alignments"]} for b in named],
                            [dict(j, left=at[j["left"]], right=at[j["right"]]) for j in jobs])
            else:
                device = device or (_DeviceRounds(dll) if first is None or first.out is None else _DeviceRounds(dll, first, first.at))
                out = device(blocks, slots, jobs)
            for j, r in zip(jobs, out):
                if r["status"] != 0:
                    raise SimplifyError(f"blocks {j['anchor']} and {j['other']}: a letter without a complement")
                del blocks["blocks"][j["left"]], blocks["blocks"][j["right"]], slots[j["other"]]
                blocks["blocks"][j["anchor"]] = {"consensus": r["consensus"], "alignments": r["members"]}
                slots[j["anchor"]] = range(len(r["members"]))
            rounds.append(given if sched is not None else [transitive[r["transitive"]] for r in res["round"]])
        b_list, p_list, n_list = planner.lists()
    finally:
        planner.close()
        if device is not None:
            if trace is not None:
                trace["zero_copy"] = list(device.zero_copy)
            device.close()
    if trace is not None:
        trace["rounds"], trace["transitive"] = rounds, lists
    # the dicts, once, from the final arrays
    out = {"paths": {}, "nodes": {}, "blocks": {bid: {"consensus": blocks["blocks"][bid]["consensus"], "alignments": {}} for bid, _, _, alive in b_list if alive}}
    for pid, off, n, _ in p_list:
        out["paths"][pid] = dict(g["paths"][pid], nodes=[x[0] for x in n_list[off:off + n]])
        for nid, pos0, pos1, b, member, rev in n_list[off:off + n]:
            out["nodes"][nid] = {"block_id": bids[b], "path_id": pid, "strand": strand(rev), "position": (pos0, pos1)}
            out["blocks"][bids[b]]["alignments"][nid] = blocks["blocks"][bids[b]]["alignments"][member]
    return out


def simplify(graph, focal_names, dll=None, schedule=None, merge=None, trace=None, topology=None, paths=None):
    """graph: a parsed pangraph JSON; focal_names: the paths to keep.  -> the simplified graph in the shape of normalize().
    schedule: explicit first rounds, [[edge, ...], ...] with edge = ((block id, strand), (block id, strand)); every round's edges must be
    transitive and share no block; behind the last of them the defined order goes on.  merge: stands in for the device call (blocks, edges as merge_blocks takes them -> its result).
    trace: a dict that receives "rounds" (the rounds taken) and "zero_copy" (per device round: its input was the previous output).
    topology: None -- the graph level is the host functions of this module; "device" -- it is pga_plan_simplify, one call per round
    (topology.py), or a callable standing in for that call (blocks, paths, nodes, sched, flags as lists -> what PlanOut.to_lists() gives);
    trace then also receives "transitive", the transitive edges of every round taken.
    paths: None -- the paths that are not focal are removed by remove_path, one after the other; "device" -- the loaded graph is packed once
    and they are removed by one pga_remove_paths call (remove.py), whose arrays the first round reads by pointer: the planner of
    topology="device" its graph, the first pga_merge_blocks call its blocks (trace["zero_copy"][0] is True); or a callable standing in for
    that call (see remove.removed_graph)."""
    g = normalize(graph)
    focal = set(focal_names)
    if paths is not None:
        from . import remove as rm
        first = rm.removed_graph(g, focal, paths, dll)
        try:
            return _simplify_removed(first, dll, schedule, merge, trace, topology)
        finally:
            first.close()
    for pid in [pid for pid in sorted(g["paths"]) if g["paths"][pid]["name"] not in focal]:
        remove_path(g, pid)
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}      # the member order of every block in the arrays
    if topology is not None:
        return _simplify_planned(g, order, dll, schedule, merge, trace, topology)
    return _simplify_rounds(g, order, dll, schedule, merge, trace)


def _simplify_removed(first, dll, schedule, merge, trace, topology):
    """simplify() behind pga_remove_paths: the same two loops, started on the arrays of that call.  The members of a block keep their
    relative order, so the member order of the arrays is still the node id order."""
    g = first.g
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    if topology is not None:
        return _simplify_planned(g, order, dll, schedule, merge, trace, topology, first)
    return _simplify_rounds(g, order, dll, schedule, merge, trace, first)


def _simplify_rounds(g, order, dll, schedule, merge, trace, first=None):
    """simplify()'s loop with the graph level on the host"""
    device = None
    rounds = []
    try:
        while True:
            transitive = find_transitive_edges(g)
            if not transitive:
                break
            if schedule is not None and len(rounds) < len(schedule):
                rnd = [tuple(map(tuple, e)) for e in schedule[len(rounds)]]
                if any(_conventional(e) not in transitive for e in rnd) or len({b for e in rnd for b in (e[0][0], e[1][0])}) != 2 * len(rnd) or not rnd:
                    raise ValueError("a round of the schedule is empty, names an edge that is not transitive, or uses a block twice")
            else:
                rnd = choose_round(transitive)
            jobs, plans = [], []
            for e in rnd:
                e = orient_merging_edge(g, e)
                pair, new = find_node_pairings(g, e)
                (a, sa), (b, sb) = e
                rc = sa != sb                                                         # merge_blocks.rs:100-111: the second block is the one complemented
                left, right, left_rc, right_rc = (a, b, False, rc) if sa == "+" else (b, a, rc, False)
                at = {n: i for i, n in enumerate(order[right])}
                jobs.append({"left": left, "right": right, "left_rc": left_rc, "right_rc": right_rc, "partner": [at[pair[n]] for n in order[left]], "anchor": a})
                plans.append((e, new))
            if merge is not None:
                named = [b for j in jobs for b in (j["left"], j["right"])]
                at = {b: i for i, b in enumerate(named)}
                res = merge([{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in named],
                            [dict(j, left=at[j["left"]], right=at[j["right"]]) for j in jobs])
            else:
                device = device or (_DeviceRounds(dll) if first is None or first.out is None else _DeviceRounds(dll, first, first.at))
                res = device(g, order, jobs)
            for j, (e, new), r in zip(jobs, plans, res):
                if r["status"] != 0:
                    raise SimplifyError(f"blocks {e[0][0]} and {e[1][0]}: a letter without a complement")
                ids = [new[n][0] for n in order[j["left"]]]
                graph_merging_update(g, e, {"consensus": r["consensus"], "alignments": dict(zip(ids, r["members"]))}, new)
                del order[e[1][0]]
                order[e[0][0]] = ids
            rounds.append(rnd)
    finally:
        if device is not None:
            if trace is not None:
                trace["zero_copy"] = list(device.zero_copy)
            device.close()
    if trace is not None:
        trace["rounds"] = rounds
    return g
