"""The graph update of a merge round on the device: `pga_apply_merge` (include/pga_align.h, pga_apply.hip) replaces every node of a cut block
by the nodes of its kept slices, makes the new nodes with their ids, and builds the block table behind the round with the member slots of
every new block -- the GraphUpdate of reweave (reweave.rs:359-401, 445-450 over pangraph.rs:68-107) and the insertion of the merged blocks
(graph_merging.rs:156-165) in one call, flat arrays in and out.  ctypes only; the HIP library does the work.

The graph is the three arrays of pangraph_amd/topology.py; the cut is the output of pga_plan_merge and pga_slice_blocks as it stands.  A
call's graph arrays are the next call's input by pointer, and pga_plan_simplify's."""
import ctypes as C

from . import batch
from .reweave import plan_interval_t
from .slice import slice_member_t, slice_res_t
from .topology import pack_lists, topo_block_t, topo_node_t, topo_path_t, unpack_lists

NONE = 0xFFFFFFFF


class apply_cut_t(C.Structure):
    _fields_ = [("block", C.c_uint32), ("n_intervals", C.c_uint32), ("first_interval", C.c_uint64)]


class apply_block_t(C.Structure):
    _fields_ = [("block", C.c_uint32), ("kind", C.c_int32), ("interval_a", C.c_uint64), ("interval_b", C.c_uint64), ("member_off", C.c_uint64)]


class apply_out_t(C.Structure):
    _fields_ = [("n_new_nodes", C.c_int64), ("n_new_blocks", C.c_int64), ("n_blocks", C.c_int64), ("n_paths", C.c_int64), ("n_nodes", C.c_int64),
                ("new_nodes", C.POINTER(topo_node_t)), ("old_node", C.POINTER(C.c_uint64)), ("new_blocks", C.POINTER(apply_block_t)),
                ("member_src", C.POINTER(C.c_uint64)), ("block_map", C.POINTER(C.c_uint32)),
                ("paths", C.POINTER(topo_path_t)), ("nodes", C.POINTER(topo_node_t)), ("blocks", C.POINTER(topo_block_t))]


def _bind(dll):
    dll.pga_apply_merge.restype = C.c_int
    dll.pga_apply_merge.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.POINTER(apply_out_t)]
    dll.pga_apply_free.restype = None
    dll.pga_apply_free.argtypes = [C.POINTER(apply_out_t)]
    dll.pga_last_error.restype = C.c_char_p


# ---------------------------------------------------------------- the cut
def pack_cut(plan, graph_index):
    """plan: a reweave.PlanOut (alive) or its to_lists(); graph_index[i]: the index in the graph's block table of the plan call's input block i
    -> (n_cut, apply_cut_t array): one record per plan.blocks[k], with that record's own first_interval and n_intervals"""
    if hasattr(plan, "out"):
        rows = [(plan.out.blocks[k].block, plan.out.blocks[k].n_intervals, plan.out.blocks[k].first_interval) for k in range(plan.out.n_blocks)]
    else:
        rows = [(b["block"], b["n_intervals"], b["first_interval"]) for b in plan["blocks"]]
    return len(rows), (apply_cut_t * max(len(rows), 1))(*[apply_cut_t(graph_index[b], n, first) for b, n, first in rows])


def pack_cut_lists(cut, intervals, slices, members):
    """cut: [(graph block index, n_intervals, first_interval)]; intervals: [{"new_block_id", "start", "end", "aligned", "is_anchor"}];
    slices: [(member_off, n_kept, n_dropped)]; members: [(member, reverse, pos_start, pos_end)] -> (n_cut, cut, intervals, slices, members) as C arrays"""
    K = (apply_cut_t * max(len(cut), 1))(*[apply_cut_t(*c) for c in cut])
    I = (plan_interval_t * max(len(intervals), 1))()
    for r, iv in zip(I, intervals):
        r.new_block_id, r.start, r.end, r.aligned, r.is_anchor, r.match = iv["new_block_id"], iv["start"], iv["end"], 1 if iv["aligned"] else 0, 1 if iv["is_anchor"] else 0, -1
    S = (slice_res_t * max(len(slices), 1))(*[slice_res_t(*s) for s in slices])
    M = (slice_member_t * max(len(members), 1))()
    for r, (member, reverse, pos_start, pos_end) in zip(M, members):
        r.member, r.reverse, r.pos_start, r.pos_end = member, 1 if reverse else 0, pos_start, pos_end
    return len(cut), K, I, S, M


# ---------------------------------------------------------------- the call
class ApplyOut:
    """the output of one call; owns its arrays until free().  `graph_args()` are the first six arguments of the next pga_apply_merge and of
    pga_plan_simplify: pointers into this output, nothing is copied.  None when the cut was empty (the graph is unchanged)."""

    def __init__(self, dll, out, keep):
        self.dll, self.out, self.keep = dll, out, keep

    def graph_args(self):
        o = self.out
        if not o.blocks:
            return None
        cast = lambda p: C.cast(p, C.c_void_p)
        return (o.n_blocks, cast(o.blocks), o.n_paths, cast(o.paths), o.n_nodes, cast(o.nodes))

    def to_lists(self, n_blocks_in=0):
        """{"new_nodes": [(node_id, pos0, pos1, block, member, reverse)], "old_node", "new_blocks": [(block, kind, interval_a, interval_b, member_off)],
        "member_src", "block_map" (n_blocks_in entries), "blocks", "paths", "nodes"}; the three graph lists are None when the cut was empty"""
        o = self.out
        n = o.n_new_nodes
        args = self.graph_args()
        blocks, paths, nodes = unpack_lists(args) if args else (None, None, None)
        return {"new_nodes": [(x.node_id, x.pos0, x.pos1, x.block, x.member, x.reverse) for x in (o.new_nodes[i] for i in range(n))],
                "old_node": o.old_node[:n] if n else [], "member_src": o.member_src[:n] if n else [],
                "new_blocks": [(x.block, x.kind, x.interval_a, x.interval_b, x.member_off) for x in (o.new_blocks[i] for i in range(o.n_new_blocks))],
                "block_map": o.block_map[:n_blocks_in] if args and n_blocks_in else [], "blocks": blocks, "paths": paths, "nodes": nodes}

    def free(self):
        if self.out is not None:
            self.dll.pga_apply_free(C.byref(self.out))
            self.out = None


def apply_merge_raw(graph_args, n_cut, cut, intervals, slices, members, dll=None, keep=None):
    """graph_args: (n_blocks, blocks, n_paths, paths, n_nodes, nodes) as C arrays or pointers (topology.pack_lists / pack_graph, an ApplyOut's or a
    topology.PlanOut's graph_args()); cut: pack_cut's array; intervals: plan.out.intervals; slices, members: the slice call's -> ApplyOut"""
    dll = dll or batch.lib()
    _bind(dll)
    out = apply_out_t()
    ptr = lambda p: C.cast(p, C.c_void_p) if p is not None else None
    if dll.pga_apply_merge(*graph_args, n_cut, ptr(cut), ptr(intervals), ptr(slices), ptr(members), C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return ApplyOut(dll, out, keep)


def apply_merge(blocks, paths, nodes, cut, intervals, slices, members, dll=None):
    """one call on lists (topology.pack_lists and pack_cut_lists) -> ApplyOut.to_lists()"""
    args = pack_lists(blocks, paths, nodes)
    K = pack_cut_lists(cut, intervals, slices, members)
    out = apply_merge_raw(args, *K, dll=dll, keep=(args, K))
    try:
        return out.to_lists(len(blocks))
    finally:
        out.free()
