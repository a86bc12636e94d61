"""graph_join on the two flat layouts: `pga_join_graphs` (include/pga_align.h, pga_join.hip) puts the child graphs of a guide-tree node into
one (graph_merging.rs:74-93, the first line of merge_graphs): the union of their blocks, paths and nodes in id order, a "Conflicting key"
refusal on a shared id.  A part is a graph in both layouts, as a CloseOut hands it on; the output is one again, so a build's graph never
leaves the two flat layouts between merges.  ctypes and numpy only; the HIP library does the work.

A `JoinOut`'s `graph_args()` are the first six arguments of pga_apply_merge, pga_plan_simplify, pga_remove_paths and the exports, its
`block_args()` the first seven of pga_assemble_blocks, pga_reconstruct, pga_merge_blocks, pga_remove_paths and pga_export_json, its `who`
the member-to-node map those entries assume: pointers, nothing is copied."""
import ctypes as C

import numpy as np

from . import batch
from . import close as cl
from .assemble import MEMBER, WHO, _ptr, _view
from .detach import DEL, INS, SUB, detach_member_t
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_block_t, rc_member_t
from .topology import topo_block_t, topo_node_t, topo_path_t, unpack_lists

COPY_CONSENSUS = 1                   # PGA_JOIN_COPY_CONSENSUS
NONE = 0xFFFFFFFF


class join_part_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int64), ("blocks", C.c_void_p), ("n_paths", C.c_int64), ("paths", C.c_void_p), ("n_nodes", C.c_int64), ("nodes", C.c_void_p),
                ("rc_blocks", C.c_void_p), ("members", C.c_void_p), ("subs", C.c_void_p), ("dels", C.c_void_p), ("inss", C.c_void_p),
                ("ins_seq", C.c_void_p), ("ins_seq_len", C.c_uint64), ("who", C.c_void_p)]


class join_out_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int64), ("n_paths", C.c_int64), ("n_nodes", C.c_int64), ("n_members", C.c_int64), ("n_parts", C.c_int64),
                ("n_subs", C.c_uint64), ("n_dels", C.c_uint64), ("n_inss", C.c_uint64), ("n_ins_letters", C.c_uint64), ("n_cons_letters", C.c_uint64),
                ("blocks", C.POINTER(topo_block_t)), ("paths", C.POINTER(topo_path_t)), ("nodes", C.POINTER(topo_node_t)),
                ("rc_blocks", C.POINTER(rc_block_t)), ("members", C.POINTER(rc_member_t)), ("subs", C.POINTER(sub_t)), ("dels", C.POINTER(del_t)),
                ("inss", C.POINTER(ins_t)), ("ins_seq", C.POINTER(C.c_char)), ("cons", C.POINTER(C.c_char)), ("who", C.POINTER(detach_member_t)),
                ("origin_part", C.POINTER(C.c_int32)), ("origin", C.POINTER(C.c_int64)), ("block_map", C.POINTER(C.c_uint32)), ("block_map_off", C.POINTER(C.c_uint64)),
                ("path_map", C.POINTER(C.c_uint32)), ("path_map_off", C.POINTER(C.c_uint64))]


class JoinError(Exception):
    """the reference panics in graph_join: a block, path or node id is present in both graphs"""


def _bind(dll):
    dll.pga_join_graphs.restype = C.c_int
    dll.pga_join_graphs.argtypes = [C.c_int32, C.c_void_p, C.c_uint32, C.POINTER(join_out_t)]
    dll.pga_join_free.restype = None
    dll.pga_join_free.argtypes = [C.POINTER(join_out_t)]
    dll.pga_join_last_ms.restype = None
    dll.pga_join_last_ms.argtypes = [C.POINTER(C.c_double)]
    dll.pga_last_error.restype = C.c_char_p


def _value(p):
    """the address behind anything assemble._ptr takes, or None"""
    p = _ptr(p)
    return p.value if isinstance(p, C.c_void_p) else p


# ---------------------------------------------------------------- the call
class JoinOut:
    """the output of one call; owns its arrays until free().  Without COPY_CONSENSUS every consensus pointer leads into the letters of the
    part its block came from, everything else is the call's own."""

    def __init__(self, dll, out, keep):
        self.dll, self.out, self.keep = dll, out, keep

    def graph_args(self):
        o = self.out
        return (o.n_blocks, _ptr(o.blocks), o.n_paths, _ptr(o.paths), o.n_nodes, _ptr(o.nodes))

    def block_args(self):
        o = self.out
        return (o.n_blocks, _ptr(o.rc_blocks), _ptr(o.members), _ptr(o.subs), _ptr(o.dels), _ptr(o.inss), _ptr(o.ins_seq))

    @property
    def who(self):
        o = self.out
        return C.cast(o.who, C.POINTER(detach_member_t * max(o.n_members, 1))).contents

    @property
    def n_ins_letters(self):
        return self.out.n_ins_letters

    def to_lists(self):
        """{"blocks", "paths", "nodes" (topology.unpack_lists), "rc_blocks": [(consensus bytes, n_members)], "counts" (members, 3), "subs", "dels", "inss" (the record
        dtypes of pangraph_amd/detach.py), "ins_seq", "who": [(node_id, reverse)], "origin_part", "origin", "block_map" / "path_map": over the input entries of all parts
        behind each other, "block_map_off" / "path_map_off": where a part's begin, "totals": the ten counts of the record}"""
        o = self.out
        blocks, paths, nodes = unpack_lists(self.graph_args())
        rc = []
        for b in range(o.n_blocks):
            at = cl._addr(o.rc_blocks[b])
            rc.append((C.string_at(at, o.rc_blocks[b].cons_len) if at and o.rc_blocks[b].cons_len else b"", o.rc_blocks[b].n_members))
        who = _view(o.who, o.n_members, WHO)
        b_off, p_off = o.block_map_off[:o.n_parts + 1], o.path_map_off[:o.n_parts + 1]
        return {"blocks": blocks, "paths": paths, "nodes": nodes, "rc_blocks": rc, "counts": _view(o.members, o.n_members, MEMBER).view(np.uint32).reshape(-1, 3),
                "subs": _view(o.subs, o.n_subs, SUB), "dels": _view(o.dels, o.n_dels, DEL), "inss": _view(o.inss, o.n_inss, INS),
                "ins_seq": C.string_at(o.ins_seq, o.n_ins_letters) if o.n_ins_letters else b"", "who": list(zip(who["node_id"].tolist(), who["reverse"].tolist())),
                "origin_part": o.origin_part[:o.n_members] if o.n_members else [], "origin": o.origin[:o.n_members] if o.n_members else [],
                "block_map": o.block_map[:b_off[-1]] if b_off[-1] else [], "block_map_off": b_off, "path_map": o.path_map[:p_off[-1]] if p_off[-1] else [], "path_map_off": p_off,
                "totals": tuple(getattr(o, f) for f, _ in join_out_t._fields_[:10])}

    def to_dicts(self):
        """per block after {"consensus", "members": [edit]} (remove.edits_to_dicts)"""
        from .remove import edits_to_dicts
        return edits_to_dicts(*self.block_args())

    def free(self):
        if self.out is not None:
            self.dll.pga_join_free(C.byref(self.out))
            self.out = None


class Tables(cl.Tables):
    """one part built from lists: the graph and block entries of close.Tables ("blocks", "paths", "nodes", "rc_blocks", "counts", "subs", "dels", "inss", "ins_seq",
    "who"), e.g. what close.graph_tables or singleton_tables give; keeps every buffer alive"""

    def graph_args(self):
        return self.graph

    @property
    def who(self):
        return self.W

    @property
    def n_ins_letters(self):
        return len(self.L)


def _part(x):
    """a part -> (graph_args, block_args, who, letter count).  x: an object with graph_args(), block_args(), who and its letter count (`n_ins_letters`, or that of its
    `out`): a CloseOut, a JoinOut, a Tables; or a tuple (object, who[, letter count]) for one that has no who of its own (a RemoveOut)"""
    who = n = None
    if isinstance(x, tuple):
        who, n = x[1], (x[2] if len(x) > 2 else None)
        x = x[0]
    if who is None:
        who = x.who
    if n is None:
        n = getattr(x, "n_ins_letters", None)
    if n is None:
        n = x.out.n_ins_letters
    return x.graph_args(), x.block_args(), who, int(n)


def pack_parts(parts):
    """parts: see _part -> the join_part_t array of the call (pointers only: the parts must stay alive)"""
    P = (join_part_t * max(len(parts), 1))()
    for k, x in enumerate(parts):
        g, b, who, n = _part(x)
        if g[0] != b[0]:
            raise ValueError(f"part {k}: the graph and the block arrays differ in their number of blocks")
        P[k].n_blocks, P[k].n_paths, P[k].n_nodes, P[k].ins_seq_len = g[0], g[2], g[4], n
        P[k].blocks, P[k].paths, P[k].nodes = _value(g[1]), _value(g[3]), _value(g[5])
        P[k].rc_blocks, P[k].members, P[k].subs, P[k].dels, P[k].inss = [_value(a) for a in b[1:6]]
        P[k].ins_seq = C.cast(C.c_char_p(b[6]), C.c_void_p).value if isinstance(b[6], bytes) else _value(b[6])
        P[k].who = _value(who)
    return P


def join_graphs_raw(parts, flags=0, dll=None, keep=None):
    """parts: see _part -> JoinOut.  The parts must live as long as the JoinOut unless COPY_CONSENSUS is given (its consensus pointers lead into them)"""
    dll = dll or batch.lib()
    _bind(dll)
    P = pack_parts(parts)
    out = join_out_t()
    if dll.pga_join_graphs(len(parts), _ptr(P), flags, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return JoinOut(dll, out, (keep, parts, P))


def join_graphs(list_of_tables, flags=0, dll=None):
    """one call on lists (a Tables dict per part) -> JoinOut.to_lists()"""
    K = [Tables(t) for t in list_of_tables]
    out = join_graphs_raw(K, flags=flags, dll=dll, keep=K)
    try:
        return out.to_lists()
    finally:
        out.free()


def last_ms(dll=None):
    """(upload, kernels, download) of the calling thread's last call, in ms on the stream's clock (measurement only)"""
    dll = dll or batch.lib()
    _bind(dll)
    ms = (C.c_double * 3)()
    dll.pga_join_last_ms(ms)
    return tuple(ms)


# ---------------------------------------------------------------- the leaves and the host restatement
def singleton_graph(index, seq, circular, reverse=False, name=None):
    """Pangraph::singleton (pangraph.rs:29-50) as a dict graph in the shape of simplify.normalize(): one block, one path, one node, all ids = index"""
    return {"blocks": {index: {"consensus": seq, "alignments": {index: {"subs": [], "dels": [], "inss": []}}}},
            "nodes": {index: {"block_id": index, "path_id": index, "strand": "-" if reverse else "+", "position": (0, 0) if circular else (0, len(seq))}},
            "paths": {index: {"nodes": [index], "tot_len": len(seq), "circular": bool(circular), "name": name}}}


def singleton_tables(index, seq, circular, reverse=False):
    """Pangraph::singleton as the tables of one part: one block, one path, one node, one member without an edit, all three ids = index, position (0, 0) when
    circular, else (0, len)"""
    seq = seq.encode("latin-1") if isinstance(seq, str) else bytes(seq)
    return {"blocks": [(index, len(seq), 1, 1)], "paths": [(index, 0, 1, bool(circular))], "nodes": [(index, 0, 0 if circular else len(seq), 0, 0, bool(reverse))],
            "rc_blocks": [(seq, 1)], "counts": [(0, 0, 0)], "subs": [], "dels": [], "inss": [], "ins_seq": b"", "who": [(index, bool(reverse))]}


def graph_join(left, right):
    """graph_join (graph_merging.rs:74-93) on dict graphs in the shape of simplify.normalize(): the union of the three maps; a shared key raises JoinError"""
    out = {}
    for f in ("blocks", "paths", "nodes"):
        shared = set(left[f]) & set(right[f])
        if shared:
            raise JoinError(f"Conflicting key: '{min(shared)}' ({f[:-1]} id)")
        out[f] = {**left[f], **right[f]}
    return out


def _graph_of(paths, a, dicts):
    """the dict graph behind the lists of a JoinOut; paths: what a path carries besides its nodes, keyed by path_id (the host's)"""
    from .remove import graph_after
    return graph_after({"paths": paths}, [b[0] for b in a[0]], a, dicts)


def merge_pair(left, right, rounds, thr_len, join=None, dll=None, **round_kw):
    """The head of merge_graphs (graph_merging.rs:26-63) on two dict graphs: graph_join, then close.self_merge_round once per match list in `rounds`
    (round_kw goes to it) -> the graph after.
    join=None: graph_join on the dicts.  join="device": the tables of both children, pga_join_graphs, the graph read off the JoinOut.
    join=callable: stands in for the call on tables: `join([tables left, tables right], flags)` returns what JoinOut.to_lists() gives."""
    if join is None:
        g = graph_join(left, right)
    else:
        from .assemble import _edits_of
        paths = {**left["paths"], **right["paths"]}
        tables = [cl.graph_tables(left)[0], cl.graph_tables(right)[0]]
        if join == "device":
            K = [Tables(t) for t in tables]
            out = join_graphs_raw(K, dll=dll, keep=K)
            try:
                g = _graph_of(paths, unpack_lists(out.graph_args()), out.to_dicts())
            finally:
                out.free()
        else:
            a = join(tables, 0)
            g = _graph_of(paths, (a["blocks"], a["paths"], a["nodes"]),
                          _edits_of({"blocks": a["rc_blocks"], "counts": a["counts"], "subs": a["subs"], "dels": a["dels"], "inss": a["inss"], "ins_seq": a["ins_seq"]}))
    for matches in rounds:
        g = cl.self_merge_round(g, matches, thr_len, dll=dll, **round_kw)
    return g
