"""The path side of `pangraph simplify` on the device: `pga_plan_simplify` (include/pga_align.h, pga_topo.hip) counts the edges of every path,
lists the transitive ones, chooses and orients a round of disjoint edges, pairs the nodes, makes the new nodes with their ids and rewrites
the paths -- find_transitive_edges, choose_round, orient_merging_edge, find_node_pairings and graph_merging_update of simplify.py for a whole
round in one call, flat arrays in and out.  ctypes only; the HIP library does the work.

The graph is three arrays: blocks in ascending id (index order is the reference's BTreeMap order), paths in ascending id, nodes path after
path with (block index, member slot).  A call's output arrays are the next call's input by pointer."""
import ctypes as C

from . import batch
from .simplify import merge_edge_t

EDGES_ONLY, COUNTS = 1, 2            # PGA_TOPO_EDGES_ONLY, PGA_TOPO_COUNTS
TILE = 1024                          # PGA_TOPO_TILE: path positions per workgroup of the splice's scan


class topo_block_t(C.Structure):
    _fields_ = [("block_id", C.c_uint64), ("cons_len", C.c_uint32), ("depth", C.c_uint32), ("alive", C.c_int32), ("pad", C.c_int32)]


class topo_path_t(C.Structure):
    _fields_ = [("path_id", C.c_uint64), ("node_off", C.c_uint64), ("n_nodes", C.c_uint32), ("circular", C.c_int32)]


class topo_node_t(C.Structure):
    _fields_ = [("node_id", C.c_uint64), ("pos0", C.c_uint64), ("pos1", C.c_uint64), ("block", C.c_uint32), ("member", C.c_uint32), ("reverse", C.c_int32), ("pad", C.c_int32)]


class topo_sched_t(C.Structure):
    _fields_ = [("b1", C.c_uint32), ("s1", C.c_int32), ("b2", C.c_uint32), ("s2", C.c_int32)]


class topo_edge_t(C.Structure):
    _fields_ = [("b1", C.c_uint32), ("b2", C.c_uint32), ("s1", C.c_int32), ("s2", C.c_int32), ("count", C.c_uint32), ("pad", C.c_uint32)]


class topo_round_t(C.Structure):
    _fields_ = [("anchor", C.c_uint32), ("other", C.c_uint32), ("anchor_rev", C.c_int32), ("other_rev", C.c_int32), ("transitive", C.c_uint32), ("pad", C.c_uint32),
                ("merge", merge_edge_t), ("partner_off", C.c_uint64)]


class topo_out_t(C.Structure):
    _fields_ = [("n_transitive", C.c_int64), ("n_counts", C.c_int64), ("n_round", C.c_int64), ("n_partner", C.c_int64), ("n_blocks", C.c_int64), ("n_paths", C.c_int64),
                ("n_nodes", C.c_int64), ("transitive", C.POINTER(topo_edge_t)), ("edge_counts", C.POINTER(topo_edge_t)), ("round", C.POINTER(topo_round_t)),
                ("partner", C.POINTER(C.c_uint32)), ("new_nodes", C.POINTER(topo_node_t)), ("old_left", C.POINTER(C.c_uint64)), ("old_right", C.POINTER(C.c_uint64)),
                ("paths", C.POINTER(topo_path_t)), ("nodes", C.POINTER(topo_node_t)), ("blocks", C.POINTER(topo_block_t))]


def _bind(dll):
    dll.pga_plan_simplify.restype = C.c_int
    dll.pga_plan_simplify.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_uint32, C.POINTER(topo_out_t)]
    dll.pga_topo_free.restype = None
    dll.pga_topo_free.argtypes = [C.POINTER(topo_out_t)]
    dll.pga_last_error.restype = C.c_char_p


# ---------------------------------------------------------------- the three arrays
def pack_lists(blocks, paths, nodes):
    """blocks: [(block_id, cons_len, depth, alive)], paths: [(path_id, node_off, n_nodes, circular)], nodes: [(node_id, pos0, pos1, block, member,
    reverse)] -> (n_blocks, B, n_paths, P, n_nodes, N), the first six arguments of pga_plan_simplify"""
    B = (topo_block_t * max(len(blocks), 1))(*[topo_block_t(b[0], b[1], b[2], 1 if b[3] else 0, 0) for b in blocks])
    P = (topo_path_t * max(len(paths), 1))(*[topo_path_t(p[0], p[1], p[2], 1 if p[3] else 0) for p in paths])
    N = (topo_node_t * max(len(nodes), 1))(*[topo_node_t(n[0], n[1], n[2], n[3], n[4], 1 if n[5] else 0, 0) for n in nodes])
    return (len(blocks), B, len(paths), P, len(nodes), N)


def pack_graph(g, order):
    """g: the graph of simplify.normalize; order: {block id: its node ids in member order} -> the arguments as pack_lists gives them"""
    bids = sorted(g["blocks"])
    at = {b: i for i, b in enumerate(bids)}
    slot = {n: k for b in bids for k, n in enumerate(order[b])}
    blocks = [(b, len(g["blocks"][b]["consensus"]), len(order[b]), 1) for b in bids]
    paths, nodes = [], []
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        paths.append((pid, len(nodes), len(p["nodes"]), p["circular"]))
        for nid in p["nodes"]:
            n = g["nodes"][nid]
            nodes.append((nid, n["position"][0], n["position"][1], at[n["block_id"]], slot[nid], n["strand"] == "-"))
    return pack_lists(blocks, paths, nodes)


def unpack_lists(args):
    """the inverse of pack_lists, for arrays or pointers (a PlanOut's graph_args())"""
    nb, B, np_, P, nn, N = args
    cast = lambda p, t: C.cast(p, C.POINTER(t))
    B, P, N = cast(B, topo_block_t), cast(P, topo_path_t), cast(N, topo_node_t)
    return ([(B[i].block_id, B[i].cons_len, B[i].depth, B[i].alive) for i in range(nb)], [(P[i].path_id, P[i].node_off, P[i].n_nodes, P[i].circular) for i in range(np_)],
            [(N[i].node_id, N[i].pos0, N[i].pos1, N[i].block, N[i].member, N[i].reverse) for i in range(nn)])


# ---------------------------------------------------------------- the call
class PlanOut:
    """the output of one call; `graph_args()` are the first six arguments of the next call: pointers into this output, nothing is copied.
    None when the round is empty (the graph is unchanged: the caller keeps its own).  Lives until free()."""

    def __init__(self, dll, out, keep):
        self.dll, self.out, self.keep = dll, out, keep
        self.n_round, self.n_transitive = out.n_round, out.n_transitive

    def graph_args(self):
        o = self.out
        if not o.n_round:
            return None
        cast = lambda p: C.cast(p, C.c_void_p)
        return (o.n_blocks, cast(o.blocks), o.n_paths, cast(o.paths), o.n_nodes, cast(o.nodes))

    def transitive(self):
        o = self.out
        return [(o.transitive[i].b1, o.transitive[i].b2, o.transitive[i].s1, o.transitive[i].s2, o.transitive[i].count) for i in range(o.n_transitive)]

    def edge_counts(self):
        o = self.out
        return [(o.edge_counts[i].b1, o.edge_counts[i].b2, o.edge_counts[i].s1, o.edge_counts[i].s2, o.edge_counts[i].count) for i in range(o.n_counts)]

    def round(self):
        o = self.out
        return [{"anchor": r.anchor, "other": r.other, "anchor_rev": r.anchor_rev, "other_rev": r.other_rev, "transitive": r.transitive,
                 "merge": (r.merge.left, r.merge.right, r.merge.left_rc, r.merge.right_rc), "partner_off": r.partner_off} for r in (o.round[i] for i in range(o.n_round))]

    def partner(self):
        return self.out.partner[:self.out.n_partner] if self.out.n_partner else []

    def to_lists(self):
        """everything as Python lists: {"transitive", "edge_counts", "round", "partner", "new_nodes", "old_left", "old_right", "blocks", "paths", "nodes"};
        the three graph lists are None when the round is empty"""
        o = self.out
        n = o.n_partner
        args = self.graph_args()
        blocks, paths, nodes = unpack_lists(args) if args else (None, None, None)
        return {"transitive": self.transitive(), "edge_counts": self.edge_counts(), "round": self.round(), "partner": list(self.partner()),
                "new_nodes": [(x.node_id, x.pos0, x.pos1, x.block, x.member, x.reverse) for x in (o.new_nodes[i] for i in range(n))],
                "old_left": o.old_left[:n] if n else [], "old_right": o.old_right[:n] if n else [], "blocks": blocks, "paths": paths, "nodes": nodes}

    def free(self):
        if self.out is not None:
            self.dll.pga_topo_free(C.byref(self.out))
            self.out = None


def plan_round_raw(graph_args, sched=None, flags=0, dll=None, keep=None):
    """graph_args: (n_blocks, blocks, n_paths, paths, n_nodes, nodes) as C arrays or pointers (pack_lists / pack_graph, or a PlanOut's graph_args());
    sched: None or [(b1, s1, b2, s2)] with block indices and strands 0 / 1 -> PlanOut"""
    dll = dll or batch.lib()
    _bind(dll)
    S = None if sched is None else (topo_sched_t * max(len(sched), 1))(*[topo_sched_t(b1, 1 if s1 else 0, b2, 1 if s2 else 0) for b1, s1, b2, s2 in sched])
    out = topo_out_t()
    if dll.pga_plan_simplify(*graph_args, 0 if sched is None else len(sched), S, flags, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return PlanOut(dll, out, keep)


def plan_round(blocks, paths, nodes, sched=None, flags=0, dll=None):
    """one round on lists (see pack_lists) -> PlanOut.to_lists()"""
    args = pack_lists(blocks, paths, nodes)
    out = plan_round_raw(args, sched, flags, dll, keep=args)
    try:
        return out.to_lists()
    finally:
        out.free()


# ---------------------------------------------------------------- what simplify(topology=...) drives
class DevicePlanner:
    """round after round on the device: the arrays of a round's output are the next round's input"""

    def __init__(self, args, dll=None):
        self.dll, self.args, self.keep, self.prev = dll, args, args, None

    def step(self, sched=None, flags=0):
        """-> {"transitive", "round", "partner"}; a round that is not empty becomes the current graph"""
        out = plan_round_raw(self.args, sched, flags, self.dll)
        try:
            res = {"transitive": out.transitive(), "round": out.round(), "partner": out.partner()}
        except BaseException:
            out.free()
            raise
        if out.n_round:
            if self.prev is not None:
                self.prev.free()
            self.prev, self.args = out, out.graph_args()
        else:
            out.free()
        return res

    def lists(self):
        return unpack_lists(self.args)

    def close(self):
        if self.prev is not None:
            self.prev.free()
            self.prev = None


class StandInPlanner:
    """the same over a callable that stands in for the device call: (blocks, paths, nodes, sched, flags) as lists -> what PlanOut.to_lists() gives.
    The graph still goes through the C arrays (pack_lists / unpack_lists) between the rounds."""

    def __init__(self, args, call):
        self.args, self.call = args, call

    def step(self, sched=None, flags=0):
        res = self.call(*unpack_lists(self.args), sched, flags)
        if res["round"]:
            self.args = pack_lists(res["blocks"], res["paths"], res["nodes"])
        return {"transitive": res["transitive"], "round": res["round"], "partner": res["partner"]}

    def lists(self):
        return unpack_lists(self.args)

    def close(self):
        pass
