"""The first step of `pangraph simplify` on the device: `pga_remove_paths` (include/pga_align.h, pga_remove.hip) is Pangraph::remove_path
(pangraph/pangraph.rs:110-132) for every path that is not kept, in one call on the flat graph of pangraph_amd/topology.py AND the block
arrays of pga_merge_blocks / pga_reconstruct: the members of the removed paths leave their blocks, blocks left empty die, nodes and paths
are compacted, the edit lists of the kept members are copied into dense arrays.  ctypes only; the HIP library does the work.

A call's `graph_args()` are the first six arguments of pga_plan_simplify (and the graph of pga_apply_merge), its `block_args()` the first
seven of pga_merge_blocks, pga_reconstruct and the exports: pointers, nothing is copied.  simplify(paths="device") chains them that way."""
import ctypes as C

from . import batch
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_block_t, rc_member_t
from .reconstruct import _Packed
from .topology import pack_graph, pack_lists, topo_block_t, topo_node_t, topo_path_t, unpack_lists

COMPACT_LETTERS = 1                  # PGA_REMOVE_COMPACT_LETTERS


class remove_out_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int64), ("n_paths", C.c_int64), ("n_nodes", C.c_int64), ("n_members", C.c_int64), ("n_dead_blocks", C.c_int64),
                ("n_subs", C.c_uint64), ("n_dels", C.c_uint64), ("n_inss", C.c_uint64), ("n_ins_letters", C.c_uint64),
                ("blocks", C.POINTER(topo_block_t)), ("paths", C.POINTER(topo_path_t)), ("nodes", C.POINTER(topo_node_t)),
                ("rc_blocks", C.POINTER(rc_block_t)), ("members", C.POINTER(rc_member_t)), ("subs", C.POINTER(sub_t)), ("dels", C.POINTER(del_t)),
                ("inss", C.POINTER(ins_t)), ("ins_seq", C.POINTER(C.c_char)), ("member_map", C.POINTER(C.c_int64)), ("path_map", C.POINTER(C.c_int32))]


def _bind(dll):
    dll.pga_remove_paths.restype = C.c_int
    dll.pga_remove_paths.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p, C.c_uint32,
                                     C.POINTER(remove_out_t)]
    dll.pga_remove_free.restype = None
    dll.pga_remove_free.argtypes = [C.POINTER(remove_out_t)]
    dll.pga_remove_last_ms.restype = None
    dll.pga_remove_last_ms.argtypes = [C.POINTER(C.c_double)]
    dll.pga_last_error.restype = C.c_char_p


def _ptr(p):
    return C.cast(p, C.c_void_p) if p is not None else None


def edits_to_dicts(n_blocks, rc_blocks, members, subs, dels, inss, ins_seq):
    """the seven block arguments (arrays or pointers) -> per block {"consensus", "members": [edit]}, edit = {"subs": [(pos, letter)], "dels":
    [(pos, len)], "inss": [(pos, seq)]}"""
    cast = lambda p, t: C.cast(p, C.POINTER(t))
    B, M, S, D, I = cast(rc_blocks, rc_block_t), cast(members, rc_member_t), cast(subs, sub_t), cast(dels, del_t), cast(inss, ins_t)
    base = C.cast(ins_seq, C.c_void_p).value or 0
    res, m, s, d, i = [], 0, 0, 0, 0
    for b in range(n_blocks):
        cons_at = C.c_void_p.from_address(C.addressof(B[b])).value                  # (the field is a c_char_p: reading it would stop at a NUL)
        cons = C.string_at(cons_at, B[b].cons_len).decode("latin-1") if B[b].cons_len and cons_at else ""
        mem = []
        for c in (M[k] for k in range(m, m + B[b].n_members)):
            mem.append({"subs": [(S[k].pos, chr(S[k].alt & 255)) for k in range(s, s + c.n_subs)], "dels": [(D[k].pos, D[k].len) for k in range(d, d + c.n_dels)],
                        "inss": [(I[k].pos, C.string_at(base + I[k].seq_off, I[k].len).decode("latin-1") if I[k].len else "") for k in range(i, i + c.n_inss)]})
            s += c.n_subs; d += c.n_dels; i += c.n_inss
        m += B[b].n_members
        res.append({"consensus": cons, "members": mem})
    return res


class RemoveOut:
    """the output of one call; owns its arrays until free().  `graph_args()` and `block_args()` are pointers into this output (the
    insertion letters are the caller's unless COMPACT_LETTERS was given), nothing is copied."""

    def __init__(self, dll, out, keep_alive, n_paths_in, n_members_in, ins_seq):
        self.dll, self.out, self.keep_alive, self.n_paths_in, self.n_members_in, self.ins_seq = dll, out, keep_alive, n_paths_in, n_members_in, ins_seq

    def graph_args(self):
        o = self.out
        return (o.n_blocks, _ptr(o.blocks), o.n_paths, _ptr(o.paths), o.n_nodes, _ptr(o.nodes))

    def block_args(self):
        o = self.out
        return (o.n_blocks, _ptr(o.rc_blocks), _ptr(o.members), _ptr(o.subs), _ptr(o.dels), _ptr(o.inss), _ptr(o.ins_seq) if o.ins_seq else _ptr(self.ins_seq))

    def to_lists(self):
        """{"blocks", "paths", "nodes" (topology.unpack_lists), "rc_blocks": [(cons_len, n_members)], "members": [(n_subs, n_dels, n_inss)], "subs": [(pos, alt)],
        "dels": [(pos, len)], "inss": [(pos, len, seq_off)], "ins_seq": bytes or None, "member_map", "path_map", "counts": the nine counts of the record}"""
        o = self.out
        blocks, paths, nodes = unpack_lists(self.graph_args())
        return {"blocks": blocks, "paths": paths, "nodes": nodes, "rc_blocks": [(o.rc_blocks[b].cons_len, o.rc_blocks[b].n_members) for b in range(o.n_blocks)],
                "members": [(o.members[m].n_subs, o.members[m].n_dels, o.members[m].n_inss) for m in range(o.n_members)],
                "subs": [(o.subs[k].pos, o.subs[k].alt) for k in range(o.n_subs)], "dels": [(o.dels[k].pos, o.dels[k].len) for k in range(o.n_dels)],
                "inss": [(o.inss[k].pos, o.inss[k].len, o.inss[k].seq_off) for k in range(o.n_inss)],
                "ins_seq": C.string_at(o.ins_seq, o.n_ins_letters) if o.ins_seq else None,
                "member_map": o.member_map[:self.n_members_in] if self.n_members_in else [], "path_map": o.path_map[:self.n_paths_in] if self.n_paths_in else [],
                "counts": tuple(getattr(o, f) for f, _ in remove_out_t._fields_[:9])}

    def to_dicts(self):
        """per block index {"consensus", "members": [edit]}: a dead block has no member"""
        return edits_to_dicts(*self.block_args())

    def free(self):
        if self.out is not None:
            self.dll.pga_remove_free(C.byref(self.out))
            self.out = None


def remove_paths_raw(graph_args, block_args, keep, flags=0, ins_seq_len=0, dll=None, keep_alive=None):
    """graph_args: (n_blocks, blocks, n_paths, paths, n_nodes, nodes) as C arrays or pointers (topology.pack_lists / pack_graph, or the
    graph_args() of an earlier output); block_args: (n_blocks, rc_blocks, members, subs, dels, inss, ins_seq) the same way (a _Packed's
    args()[:7], a MergeOut's graph_args()); keep: one truth value per path, or a C array of uint8 -> RemoveOut"""
    dll = dll or batch.lib()
    _bind(dll)
    n_paths = graph_args[2]
    if keep is not None and not isinstance(keep, C.Array):
        keep = (C.c_uint8 * max(len(keep), 1))(*[1 if k else 0 for k in keep])
    n_blocks, rc_blocks = block_args[0], block_args[1]
    if n_blocks != graph_args[0]:
        raise ValueError("the graph and the block arrays differ in their number of blocks")
    R = C.cast(rc_blocks, C.POINTER(rc_block_t)) if rc_blocks is not None else None
    n_members_in = sum(R[b].n_members for b in range(n_blocks)) if R else 0
    out = remove_out_t()
    if dll.pga_remove_paths(*[_ptr(a) if not isinstance(a, int) else a for a in graph_args], *[_ptr(a) for a in block_args[1:7]], ins_seq_len, _ptr(keep), flags, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return RemoveOut(dll, out, (keep_alive, graph_args, block_args, keep), n_paths, n_members_in, block_args[6])


def last_ms(dll=None):
    """(upload, kernels, download) of the calling thread's last call, in ms on the stream's clock (measurement only)"""
    dll = dll or batch.lib()
    _bind(dll)
    ms = (C.c_double * 3)()
    dll.pga_remove_last_ms(ms)
    return tuple(ms)


# ---------------------------------------------------------------- the graph level
def pack_blocks(g, order):
    """every block of the graph in id order, its members in the order of order[block id] -> a _Packed (its args()[:7] are the block arguments)"""
    return _Packed([{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in sorted(g["blocks"])], [])


def graph_after(g, bids, lists, dicts):
    """the dict graph behind a call: g the graph before (for what a path carries besides its nodes), bids the id of every block index,
    lists = (blocks, paths, nodes) after, dicts the blocks after as to_dicts() gives them"""
    b_list, p_list, n_list = lists
    out = {"paths": {}, "nodes": {}, "blocks": {bids[i]: {"consensus": dicts[i]["consensus"], "alignments": {}} for i, b in enumerate(b_list) if b[3]}}
    for pid, off, n, _ in p_list:
        out["paths"][pid] = dict(g["paths"][pid], nodes=[x[0] for x in n_list[off:off + n]])
        for nid, pos0, pos1, b, member, rev in n_list[off:off + n]:
            out["nodes"][nid] = {"block_id": bids[b], "path_id": pid, "strand": "-" if rev else "+", "position": (pos0, pos1)}
            out["blocks"][bids[b]]["alignments"][nid] = dicts[b]["members"][member]
    return out


class Removed:
    """what simplify(paths=...) goes on with: the graph after as dicts (read back once), and the arrays the first round takes by pointer.
    `bids`: the id of every block index (the indices of the loaded graph: blocks do not move); `args`: the six graph arguments after;
    graph_args() / free(): the face _DeviceRounds needs of a previous output (the block arrays; freed by close(), not by the round)."""

    def __init__(self, g, bids, args, out, keep_alive=None):
        self.g, self.bids, self.args, self.out, self.keep_alive = g, bids, args, out, keep_alive
        self.at = {b: i for i, b in enumerate(bids) if b in g["blocks"]}

    def graph_args(self):
        return self.out.block_args()

    def free(self):
        pass

    def close(self):
        if self.out is not None:
            self.out.free()
            self.out = None


def removed_graph(g, focal, paths="device", dll=None, flags=0):
    """g: a graph of simplify.normalize; focal: the names of the paths that stay; paths: "device", or a callable standing in for the call:
    (blocks, paths, nodes, block dicts, keep) -> {"blocks", "paths", "nodes", "dicts"} -> Removed.  The loaded graph is packed once: all
    blocks in id order, the members of a block in node id order."""
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    bids = sorted(g["blocks"])
    keep = [g["paths"][pid]["name"] in focal for pid in sorted(g["paths"])]
    args = pack_graph(g, order)
    if paths == "device":
        K = pack_blocks(g, order)
        out = remove_paths_raw(args, K.args()[:7], keep, flags, C.sizeof(K.L), dll, keep_alive=K)
        try:
            after = graph_after(g, bids, unpack_lists(out.graph_args()), out.to_dicts())
        except BaseException:
            out.free()
            raise
        return Removed(after, bids, out.graph_args(), out)
    res = paths(*unpack_lists(args), [{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in bids], keep)
    lists = (res["blocks"], res["paths"], res["nodes"])
    args = pack_lists(*lists)
    return Removed(graph_after(g, bids, unpack_lists(args), res["dicts"]), bids, args, None, keep_alive=args)


def remove_paths(graph, focal_names, dll=None, flags=0):
    """graph: a parsed pangraph JSON (or a normalized graph); focal_names: the paths that stay -> the graph in the shape of simplify.normalize
    after simplify.remove_path of every other path"""
    from .simplify import normalize
    R = removed_graph(normalize(graph), set(focal_names), "device", dll, flags)
    try:
        return R.g
    finally:
        R.close()
