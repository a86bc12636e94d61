"""The tail of a self-merge round on the two flat layouts: `pga_close_round` (include/pga_align.h, pga_close.hip) folds what
pga_detach_unaligned -> pga_reconsensus -> pga_detach_unaligned returned for the merged blocks back into the flat graph of pga_plan_simplify
and the block arrays of pga_assemble_blocks (self_merge, graph_merging.rs:153-169; reconsensus_graph, reconsensus.rs:46-91): unaligned
members become singleton blocks, their nodes move there, every merged block gets its consensus and member edits after the reconsensus.
ctypes and numpy only; the HIP library does the work.

A `CloseOut`'s `graph_args()` are the first six arguments of the next pga_apply_merge, of pga_plan_simplify, pga_remove_paths and the
exports, its `block_args()` the first seven of the next pga_assemble_blocks, of pga_reconstruct, pga_merge_blocks, pga_remove_paths and
pga_export_json, its `who` the member-to-node map those entries assume: pointers, nothing is copied."""
import ctypes as C

import numpy as np

from . import batch
from .assemble import MEMBER, WHO, _ptr, _records, _view
from .detach import DEL, INS, SUB, detach_member_t, detach_orphan_t, detach_out_t
from .mapvar import del_t, ins_t, res_t, sub_t
from .reconsensus import rc_block_res_t, rc_block_t, rc_member_t, rc_out_t
from .topology import pack_lists, topo_block_t, topo_node_t, topo_path_t, unpack_lists

COPY_CONSENSUS = 1                   # PGA_CLOSE_COPY_CONSENSUS
TILE = 1024                          # PGA_ASSEMBLE_TILE: positions per workgroup of the scans and of the element copies
NONE = 0xFFFFFFFF
ORPHAN = np.dtype([("member", "<u8"), ("node_id", "<u8"), ("block_id", "<u8"), ("block", "<u4"), ("len", "<u4"), ("status", "<i4"), ("pad", "<i4")])
assert ORPHAN.itemsize == C.sizeof(detach_orphan_t)


class close_out_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int64), ("n_paths", C.c_int64), ("n_nodes", C.c_int64), ("n_members", C.c_int64), ("n_orphans", C.c_int64),
                ("n_subs", C.c_uint64), ("n_dels", C.c_uint64), ("n_inss", C.c_uint64), ("n_ins_letters", C.c_uint64), ("n_cons_letters", C.c_uint64),
                ("blocks", C.POINTER(topo_block_t)), ("paths", C.POINTER(topo_path_t)), ("nodes", C.POINTER(topo_node_t)),
                ("rc_blocks", C.POINTER(rc_block_t)), ("members", C.POINTER(rc_member_t)), ("subs", C.POINTER(sub_t)), ("dels", C.POINTER(del_t)),
                ("inss", C.POINTER(ins_t)), ("ins_seq", C.POINTER(C.c_char)), ("cons", C.POINTER(C.c_char)), ("who", C.POINTER(detach_member_t)),
                ("origin", C.POINTER(C.c_int64)), ("block_map", C.POINTER(C.c_uint32)), ("kinds", C.POINTER(C.c_int32)), ("orphans", C.POINTER(detach_orphan_t))]


class CloseError(Exception):
    """the reference returns Err in the tail of the round: a block's reconsensus failed, a member could not be realigned, an orphan's
    sequence could not be built"""


def _bind(dll):
    dll.pga_close_round.restype = C.c_int
    dll.pga_close_round.argtypes = [C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(close_out_t)]
    dll.pga_close_free.restype = None
    dll.pga_close_free.argtypes = [C.POINTER(close_out_t)]
    dll.pga_close_last_ms.restype = None
    dll.pga_close_last_ms.argtypes = [C.POINTER(C.c_double)]
    dll.pga_rc_detach_args.restype = C.c_int
    dll.pga_rc_detach_args.argtypes = [C.c_int64] + [C.c_void_p] * 6
    dll.pga_last_error.restype = C.c_char_p


def _addr(struct):
    """the pointer value of a structure's first field (a c_char_p field read as such would stop at a NUL)"""
    return C.c_void_p.from_address(C.addressof(struct)).value


# ---------------------------------------------------------------- the call
class CloseOut:
    """the output of one call; owns its arrays until free().  Without COPY_CONSENSUS the consensus pointers of the blocks the round did not
    rewrite lead into the caller's letters, everything else is the call's own."""

    def __init__(self, dll, out, n_blocks_in, n_upd, keep):
        self.dll, self.out, self.n_blocks_in, self.n_upd, self.keep = dll, out, n_blocks_in, n_upd, keep

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

    def to_lists(self):
        """{"blocks", "paths", "nodes" (topology.unpack_lists), "rc_blocks": [(consensus bytes, n_members)], "counts" (members, 3), "subs", "dels", "inss" (the record
        dtypes of pangraph_amd/detach.py), "ins_seq", "who": [(node_id, reverse)], "origin", "block_map", "kinds", "orphans": [(member, node_id, block_id, block, len,
        status)], "totals": the ten counts of the record}"""
        o = self.out
        blocks, paths, nodes = unpack_lists(self.graph_args())
        rc = []
        for b in range(o.n_blocks):
            at = _addr(o.rc_blocks[b])
            rc.append((C.string_at(at, o.rc_blocks[b].cons_len) if at and o.rc_blocks[b].cons_len else b"", o.rc_blocks[b].n_members))
        who, orph = _view(o.who, o.n_members, WHO), _view(o.orphans, o.n_orphans, ORPHAN)
        return {"blocks": blocks, "paths": paths, "nodes": nodes, "rc_blocks": rc, "counts": _view(o.members, o.n_members, MEMBER).view(np.uint32).reshape(-1, 3),
                "subs": _view(o.subs, o.n_subs, SUB), "dels": _view(o.dels, o.n_dels, DEL), "inss": _view(o.inss, o.n_inss, INS),
                "ins_seq": C.string_at(o.ins_seq, o.n_ins_letters) if o.n_ins_letters else b"", "who": list(zip(who["node_id"].tolist(), who["reverse"].tolist())),
                "origin": o.origin[:o.n_members] if o.n_members else [], "block_map": o.block_map[:self.n_blocks_in] if self.n_blocks_in else [],
                "kinds": o.kinds[:self.n_upd] if self.n_upd else [],
                "orphans": [tuple(int(r[f]) for f in ("member", "node_id", "block_id", "block", "len", "status")) for r in orph],
                "totals": tuple(getattr(o, f) for f, _ in close_out_t._fields_[:10])}

    def to_dicts(self):
        """per block after {"consensus", "members": [edit]} (remove.edits_to_dicts)"""
        from .remove import edits_to_dicts
        return edits_to_dicts(*self.block_args())

    def free(self):
        if self.out is not None:
            self.dll.pga_close_free(C.byref(self.out))
            self.out = None


def close_round_raw(graph_args, block_args, ins_seq_len, who, upd, detached, rc, rc_ins_seq_len, redetached, flags=0, dll=None, keep=None):
    """graph_args: (n_blocks, blocks, n_paths, paths, n_nodes, nodes), the graph of an apply.ApplyOut; block_args: (n_blocks, rc_blocks, members, subs,
    dels, inss, ins_seq), the block_args() of the default assemble.AssembleOut, ins_seq_len its letter count, who its who; upd: the graph
    indices of the updated blocks (a sequence or a uint32 array); detached / redetached: the detach_out_t of the two pga_detach_unaligned
    calls (or DetachOut); rc: the rc_out_t between them, rc_ins_seq_len the letters its read members hold -> CloseOut"""
    dll = dll or batch.lib()
    _bind(dll)
    U = np.ascontiguousarray(np.asarray(upd, np.uint32))
    d1, d2 = getattr(detached, "out", detached), getattr(redetached, "out", redetached)
    out = close_out_t()
    if dll.pga_close_round(graph_args[0], _ptr(graph_args[1]), graph_args[2], _ptr(graph_args[3]), graph_args[4], _ptr(graph_args[5]),
                           *[_ptr(a) for a in block_args[1:7]], ins_seq_len, _ptr(who), len(U), _ptr(U), _ptr(d1), _ptr(rc), rc_ins_seq_len, _ptr(d2), flags, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return CloseOut(dll, out, graph_args[0], len(U), (keep, graph_args, block_args, who, U, detached, rc, redetached))


def rc_detach_args(n_upd, detached, who_merged, rc, dll=None):
    """the first arguments of the second pga_detach_unaligned call from a pga_rc_out_t (host only): detached: the first call's detach_out_t (or
    DetachOut), who_merged: the detach_member_t array it was given -> (blocks, members, who2); rc.subs, rc.dels, rc.inss and rc.ins_seq are
    dense in member order and go into that call by pointer"""
    dll = dll or batch.lib()
    _bind(dll)
    d1 = getattr(detached, "out", detached)
    n_kept = sum(d1.blocks[j].n_members for j in range(n_upd))
    B, M, W = (rc_block_t * max(n_upd, 1))(), (rc_member_t * max(n_kept, 1))(), (detach_member_t * max(n_kept, 1))()
    if dll.pga_rc_detach_args(n_upd, _ptr(d1), _ptr(who_merged), _ptr(rc), _ptr(B), _ptr(M), _ptr(W)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return B, M, W


def last_ms(dll=None):
    """(upload, kernels, download) of the calling thread's last call, in ms on the stream's clock (measurement only)"""
    dll = dll or batch.lib()
    _bind(dll)
    ms = (C.c_double * 3)()
    dll.pga_close_last_ms(ms)
    return tuple(ms)


# ---------------------------------------------------------------- the list level
class _Detached:
    """a detach_out_t from lists: d = {"n_members": per input block, "member_map", "orphans": [(member, node_id, block_id, len, status, letters)],
    and for the second call "counts", "subs", "dels", "inss"}"""

    def __init__(self, d):
        kept, orph = list(d["n_members"]), d["orphans"]
        nb = len(kept) + len(orph)
        at, parts = [], bytearray()
        for o in orph:
            at.append(len(parts))
            parts += bytes(o[5]) + b"\0" * (-len(o[5]) % 16)
        self.cons = C.create_string_buffer(bytes(parts), max(len(parts), 1))
        self.B = (rc_block_t * max(nb, 1))()
        for j, n in enumerate(kept):
            self.B[j].n_members = n
        self.O = np.zeros(len(orph), ORPHAN)
        for k, o in enumerate(orph):
            r = self.B[len(kept) + k]
            C.c_void_p.from_address(C.addressof(r)).value = C.addressof(self.cons) + at[k]
            r.cons_len, r.n_members = len(o[5]), 1
            self.O[k] = (o[0], o[1], o[2], len(kept) + k, o[3], o[4], 0)
        self.map = np.ascontiguousarray(np.asarray(d["member_map"], np.int64))
        self.M = np.ascontiguousarray(np.asarray(d.get("counts", np.zeros((0, 3))), np.uint32).reshape(-1, 3))
        self.S, self.D, self.I = _records(d.get("subs", []), SUB), _records(d.get("dels", []), DEL), _records(d.get("inss", []), INS)
        o = self.out = detach_out_t()
        o.n_blocks, o.n_orphans = nb, len(orph)
        o.blocks = C.cast(self.B, C.POINTER(rc_block_t)); o.cons = C.cast(self.cons, C.POINTER(C.c_char))
        for name, a, ct in (("members", self.M, rc_member_t), ("subs", self.S, sub_t), ("dels", self.D, del_t), ("inss", self.I, ins_t), ("member_map", self.map, C.c_int64),
                            ("orphans", self.O, detach_orphan_t)):
            if a.size:
                setattr(o, name, C.cast(C.c_void_p(a.ctypes.data), C.POINTER(ct)))


class Tables:
    """the C view of one call's input given as lists and numpy arrays; keeps every buffer alive.  t:
      "blocks", "paths", "nodes": the graph as topology.pack_lists takes it; "rc_blocks": [(consensus bytes, n_members)] per graph block, "counts": (members, 3),
      "subs" / "dels" / "inss": SUB / DEL / INS records, "ins_seq": bytes, "who": [(node_id, reverse)] per member; "upd": [graph index];
      "detached": {"n_members", "member_map", "orphans": [(member, node_id, block_id, len, status, letters)]};
      "rc": {"blocks": [(kind, consensus bytes)], "status": per member the first detach kept, "ins_seq": bytes}; "rc_ins_seq_len": default len(rc ins_seq);
      "redetached": as "detached", with "counts", "subs", "dels", "inss" of the members it kept (seq_off into the rc's letters)."""

    def __init__(self, t):
        self.graph = pack_lists(t["blocks"], t["paths"], t["nodes"])
        nb = len(t["rc_blocks"])
        self.cons = [bytes(c) for c, _ in t["rc_blocks"]]
        self.B = (rc_block_t * max(nb, 1))()
        for i, (c, n) in enumerate(t["rc_blocks"]):
            self.B[i].consensus = self.cons[i]; self.B[i].cons_len = len(self.cons[i]); self.B[i].n_members = n
        self.n_blocks = nb
        self.M = np.ascontiguousarray(np.asarray(t["counts"], np.uint32).reshape(-1, 3))
        self.S, self.D, self.I = _records(t["subs"], SUB), _records(t["dels"], DEL), _records(t["inss"], INS)
        self.L = bytes(t["ins_seq"])
        self.W = np.zeros(len(t["who"]), WHO)
        if len(t["who"]):
            self.W["node_id"], self.W["reverse"] = [w[0] for w in t["who"]], [1 if w[1] else 0 for w in t["who"]]
        self.upd = list(t.get("upd", []))
        self.d1 = self.d2 = self.rc = None
        self.rc_len = 0
        if self.upd or t.get("detached") is not None:
            self.d1, self.d2 = _Detached(t["detached"]), _Detached(t["redetached"])
            r = t["rc"]
            at, parts = [], bytearray()
            for _, c in r["blocks"]:
                at.append(len(parts))
                parts += bytes(c) + b"\0" * (-len(c) % 16)
            self.rc_cons = C.create_string_buffer(bytes(parts), max(len(parts), 1))
            self.RB = (rc_block_res_t * max(len(r["blocks"]), 1))()
            for j, (kind, c) in enumerate(r["blocks"]):
                self.RB[j].kind, self.RB[j].cons_len, self.RB[j].cons_off = kind, len(c), at[j]
            self.RM = (res_t * max(len(r["status"]), 1))()
            for m, s in enumerate(r["status"]):
                self.RM[m].status = s
            self.RL = bytes(r["ins_seq"])
            self.rc = rc_out_t()
            self.rc.blocks = C.cast(self.RB, C.POINTER(rc_block_res_t)); self.rc.members = C.cast(self.RM, C.POINTER(res_t))
            self.rc.cons = C.cast(self.rc_cons, C.POINTER(C.c_char))
            if self.RL:
                self.rc.ins_seq = C.cast(C.c_char_p(self.RL), C.POINTER(C.c_char))
            self.rc_len = t.get("rc_ins_seq_len", len(self.RL))

    def block_args(self):
        return (self.n_blocks, self.B, self.M, self.S, self.D, self.I, self.L)

    def call_args(self):
        """the positional arguments of close_round_raw"""
        return (self.graph, self.block_args(), len(self.L), self.W, self.upd, self.d1.out if self.d1 else None, self.rc, self.rc_len, self.d2.out if self.d2 else None)


def close_round(t, flags=0, dll=None):
    """one call on lists (Tables) -> CloseOut.to_lists()"""
    K = Tables(t)
    out = close_round_raw(*K.call_args(), flags=flags, dll=dll, keep=K)
    try:
        return out.to_lists()
    finally:
        out.free()


# ---------------------------------------------------------------- the graph level: a whole self-merge round (graph_merging.rs:141-169)
def _host_merge(g, matches, thr_len, solve, dll, **stand_ins):
    """assemble.merge_round(blocks=None) -- reweave, solve_promise for every promise, the union of the anchor members with the re-aligned
    append members -- returning also what that function keeps to itself: the ids of the merged blocks, in promise order"""
    from .assemble import MergeError
    from .reweave import reweave
    g, promises = reweave(g, matches, thr_len, dll=dll, **stand_ins)
    order = [sorted(q["append"]["alignments"]) for q in promises]
    rows = solve([(q["anchor"]["consensus"], q["append"]["consensus"], q["reverse"], [(ln, kind) for kind, ln in q["cigar"]], [q["append"]["alignments"][n] for n in nids])
                  for q, nids in zip(promises, order)])
    for q, nids, res in zip(promises, order, rows):
        merged = {"consensus": q["anchor"]["consensus"], "alignments": dict(q["anchor"]["alignments"])}
        for k, (nid, r) in enumerate(zip(nids, res)):
            if r["status"] != 0:
                raise MergeError(f"promise {q['new_block_id']}, member {k}: status {r['status']}")
            merged["alignments"][nid] = {"subs": list(r["subs"]), "dels": list(r["dels"]), "inss": list(r["inss"])}
        g["blocks"][q["new_block_id"]] = merged
    return g, sorted(q["new_block_id"] for q in promises)


def _host_tail(g, merged, dll, detach=None, rc=None):
    """the tail on dicts: detach_unaligned_nodes, reconsensus_graph's block replacement, detach_unaligned_nodes on the realigned blocks"""
    from .detach import detach_graph
    from .reconsensus import reconsensus
    g = detach_graph(g, merged, dll=dll, detach=detach)
    order = [sorted(g["blocks"][b]["alignments"]) for b in merged]
    res = (rc or (lambda bl: reconsensus(bl, dll=dll)))([(g["blocks"][b]["consensus"], [g["blocks"][b]["alignments"][n] for n in nodes]) for b, nodes in zip(merged, order)])
    realigned = []
    for b, nodes, (kind, cons, edits, _, status) in zip(merged, order, res):
        if kind < 0:
            raise CloseError(f"block {b}: the reconsensus failed with kind {kind}")
        for k, s in enumerate(status):
            if s != 0:
                raise CloseError(f"block {b}, member {k}: status {s}")
        if kind:
            g["blocks"][b] = {"consensus": cons, "alignments": {n: {"subs": list(e["subs"]), "dels": list(e["dels"]), "inss": list(e["inss"])} for n, e in zip(nodes, edits)}}
        if kind == 2:
            realigned.append(b)
    return detach_graph(g, realigned, dll=dll, detach=detach)


def graph_tables(g, before_ids=()):
    """a dict graph -> the graph and block entries of Tables, and the node order of its members: blocks by ascending id, members by ascending node id"""
    from .assemble import _EditPool
    bids = sorted(g["blocks"])
    order = {b: sorted(g["blocks"][b]["alignments"]) for b in bids}
    at = {b: i for i, b in enumerate(bids)}
    slot = {n: k for b in bids for k, n in enumerate(order[b])}
    paths, nodes = [], []
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        paths.append((pid, len(nodes), len(p["nodes"]), p["circular"]))
        nodes += [(nid, g["nodes"][nid]["position"][0], g["nodes"][nid]["position"][1], at[g["nodes"][nid]["block_id"]], slot[nid], g["nodes"][nid]["strand"] == "-") for nid in p["nodes"]]
    pool = _EditPool()
    counts = [pool.add(g["blocks"][b]["alignments"][n])[:3] for b in bids for n in order[b]]
    return {"blocks": [(b, len(g["blocks"][b]["consensus"]), len(order[b]), 1) for b in bids], "paths": paths, "nodes": nodes,
            "rc_blocks": [(g["blocks"][b]["consensus"].encode("latin-1"), len(order[b])) for b in bids], "counts": counts, "subs": pool.subs, "dels": pool.dels,
            "inss": pool.inss, "ins_seq": bytes(pool.letters), "who": [(n, g["nodes"][n]["strand"] == "-") for b in bids for n in order[b]]}, order


def _list_tail(g, merged, close, dll, detach=None, rc=None):
    """the tail on lists: the tables of one pga_close_round call built from the list level of the detach and reconsensus entries (or their
    stand-ins), `close(tables, flags)` in place of the call, its lists read back into the dicts"""
    from .assemble import _EditPool, _edits_of
    from .detach import detach_unaligned
    from .reconsensus import reconsensus
    from .remove import graph_after
    t, order = graph_tables(g)
    at = {b[0]: i for i, b in enumerate(t["blocks"])}
    detach = detach or (lambda bl, w: detach_unaligned(bl, w, dll))
    blocks = [{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in merged]
    who = [[(n, g["nodes"][n]["strand"] == "-") for n in order[b]] for b in merged]
    d1 = detach(blocks, who)
    n_upd, gone = len(merged), {o["member"] for o in d1["orphans"]}
    kept = d1["blocks"][:n_upd]
    flat_who = [w for blk in who for w in blk]
    who2, m = [], 0
    for blk in who:
        who2.append([w for k, w in enumerate(blk) if m + k not in gone])
        m += len(blk)
    res = (rc or (lambda bl: reconsensus(bl, dll=dll)))([(b["consensus"], b["members"]) for b in kept])
    for b, (kind, _, _, _, status) in zip(merged, res):
        if kind < 0:
            raise CloseError(f"block {b}: the reconsensus failed with kind {kind}")
        for k, s in enumerate(status):
            if s != 0:
                raise CloseError(f"block {b}, member {k}: status {s}")
    d2 = detach([{"consensus": cons, "members": edits} for _, cons, edits, _, _ in res], who2)
    pool = _EditPool()
    counts2 = [pool.add(e)[:3] for b in d2["blocks"][:n_upd] for e in b["members"]]
    for d in (d1, d2):
        for o in d["orphans"]:
            if o["status"] != 0:
                raise CloseError(f"node {o['node_id']}: its sequence could not be built (status {o['status']})")
    rows = lambda d: [(o["member"], o["node_id"], o["block_id"], o["len"], o["status"], o["seq"].encode("latin-1")) for o in d["orphans"]]
    t.update({"upd": [at[b] for b in merged],
              "detached": {"n_members": [len(b["members"]) for b in kept], "member_map": d1["member_map"], "orphans": rows(d1)},
              "rc": {"blocks": [(kind, cons.encode("latin-1")) for kind, cons, _, _, _ in res], "status": [s for r in res for s in r[4]], "ins_seq": bytes(pool.letters)},
              "redetached": {"n_members": [len(b["members"]) for b in d2["blocks"][:n_upd]], "member_map": d2["member_map"], "orphans": rows(d2), "counts": counts2,
                             "subs": pool.subs, "dels": pool.dels, "inss": pool.inss}})
    a = close(t, 0)
    arrays = {"blocks": a["rc_blocks"], "counts": a["counts"], "subs": a["subs"], "dels": a["dels"], "inss": a["inss"], "ins_seq": a["ins_seq"]}
    return graph_after(g, [b[0] for b in a["blocks"]], (a["blocks"], a["paths"], a["nodes"]), _edits_of(arrays))


def device_tail(g, graph_args, o, upd, dll=None, params=None, flags=0, tap=None):
    """The tail of a round by pointer: pga_detach_unaligned -> pga_reconsensus -> pga_rc_detach_args -> pga_detach_unaligned ->
    pga_close_round.  g: the dict graph of the same round (for what a path carries besides its nodes); graph_args: the six graph arguments;
    o: the block arrays with who and their counts, an assemble_out_t (the default output of pga_assemble_blocks, or the same fields filled
    from other arrays); upd: the graph indices of the merged blocks; tap: called with the CloseOut while it is alive -> the dict graph after"""
    from . import mapvar
    from .detach import detach_unaligned_raw
    from .remove import graph_after
    dll = dll or batch.lib()
    n_upd = len(upd)
    n_mem = np.array([o.blocks[b].n_members for b in range(o.n_blocks)], np.int64)
    first = np.concatenate([[0], np.cumsum(n_mem)])
    counts = _view(o.members, o.n_members, MEMBER)
    c = counts.view(np.uint32).reshape(-1, 3).astype(np.int64)
    off = np.zeros((o.n_members + 1, 3), np.int64)
    off[1:] = np.cumsum(c, axis=0)
    spans = [(int(first[b]), int(first[b + 1])) for b in upd]
    cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dt)
    take = lambda ptr, n, dt, col: cat([_view(ptr, n, dt)[off[a, col]:off[z, col]] for a, z in spans], dt)
    M, S, D, I = cat([counts[a:z] for a, z in spans], MEMBER), take(o.subs, o.n_subs, SUB, 0), take(o.dels, o.n_dels, DEL, 1), take(o.inss, o.n_inss, INS, 2)
    W = cat([_view(o.who, o.n_members, WHO)[a:z] for a, z in spans], WHO)
    B = (rc_block_t * max(n_upd, 1))()
    for j, b in enumerate(upd):
        C.c_void_p.from_address(C.addressof(B[j])).value = _addr(o.blocks[b])
        B[j].cons_len, B[j].n_members = o.blocks[b].cons_len, o.blocks[b].n_members
    WM = (detach_member_t * max(len(W), 1)).from_buffer_copy(W.tobytes() if len(W) else bytes(C.sizeof(detach_member_t)))
    d1 = detach_unaligned_raw((n_upd, B, _ptr(M), _ptr(S), _ptr(D), _ptr(I), _ptr(o.ins_seq)), WM, dll, keep=(M, S, D, I))
    rc = rc_out_t()
    d2 = res = None
    dll.pga_reconsensus.restype = C.c_int
    dll.pga_reconsensus.argtypes = [C.c_int64] + [C.c_void_p] * 8
    dll.pga_rc_free.argtypes = [C.c_void_p]
    try:
        prm = params or mapvar.params()
        if dll.pga_reconsensus(n_upd, *[_ptr(a) for a in d1.graph_args(_ptr(o.ins_seq))[1:]], C.byref(prm), C.byref(rc)) != 0:
            raise batch.PgaError(dll.pga_last_error().decode())
        n_kept = sum(d1.out.blocks[j].n_members for j in range(n_upd))
        rc_len = sum(rc.members[m].n_ins_bases for m in range(n_kept))
        B2, M2, W2 = rc_detach_args(n_upd, d1, WM, rc, dll)
        d2 = detach_unaligned_raw((n_upd, B2, M2, _ptr(rc.subs), _ptr(rc.dels), _ptr(rc.inss), _ptr(rc.ins_seq)), W2, dll)
        try:
            block_args = (o.n_blocks, _ptr(o.blocks), _ptr(o.members), _ptr(o.subs), _ptr(o.dels), _ptr(o.inss), _ptr(o.ins_seq))
            res = close_round_raw(graph_args, block_args, o.n_ins_letters, _ptr(o.who), upd, d1, rc, rc_len, d2, flags=flags, dll=dll)
        except batch.PgaError as e:
            if "status other than 0" in str(e) or "the reconsensus failed" in str(e):              # (an orphan's status among them)
                raise CloseError(str(e)) from None
            raise
        if tap is not None:
            tap(res)
        lists = unpack_lists(res.graph_args())
        return graph_after(g, [b[0] for b in lists[0]], lists, res.to_dicts())
    finally:
        for x in (res, d2):
            if x is not None:
                x.free()
        dll.pga_rc_free(C.byref(rc))
        d1.free()


def _device_tail(g, dll, params=None, flags=0, tap=None):
    """-> the tap of assemble._device_round that runs device_tail on the arrays of the round, and the cell its graph is left in"""
    cell = {}

    def run(K, graph_args, out, applied):
        ap = applied.out
        upd = [ap.new_blocks[e].block for e in range(ap.n_new_blocks) if ap.new_blocks[e].kind == 1]
        cell["graph"] = device_tail(g, applied.graph_args(), out.out, upd, dll, params, flags, (lambda res: tap(res, applied, out)) if tap is not None else None)

    return run, cell


def self_merge_round(graph, matches, thr_len, close=None, solve=None, dll=None, detach=None, rc=None, tap=None, **stand_ins):
    """One whole self-merge round on a graph in the shape of simplify.normalize(): assemble.merge_round (reweave, solve_promise, the merged
    blocks), then the tail of self_merge (graph_merging.rs:153-169) and reconsensus_graph (reconsensus.rs:46-91) -> the graph after.
    close=None: the round of merge_round(blocks=None) (restated in _host_merge, which also returns the merged block ids), the tail on dicts (detach.detach_graph, reconsensus.reconsensus, detach_graph on the kind-2
    blocks); detach= / rc= stand in for those two device calls (as detach_graph and reconsensus take and give them).
    close="device": merge_round's device chain up to pga_assemble_blocks, then pga_detach_unaligned -> pga_reconsensus ->
    pga_detach_unaligned -> pga_close_round by pointer on the same arrays, the graph read off the CloseOut once at the end
    (tap: called with (CloseOut, ApplyOut, AssembleOut) while they are alive).
    close=callable: stands in for the pga_close_round call: `close(tables, flags)` gets the input of one call as close.Tables takes it and
    returns what CloseOut.to_lists() gives; the tables are built from the list level of the detach and reconsensus entries (or detach= / rc=).
    A block or member the reference fails on raises CloseError in every mode."""
    from . import assemble as asm
    if close == "device":
        dll = dll or batch.lib()
        run, cell = _device_tail(graph, dll, tap=tap)
        g = asm._device_round(graph, matches, thr_len, dll, tap=run)
        return cell.get("graph", g)
    if solve is None:
        from .promise import solve_promises
        solve = lambda promises: solve_promises(promises, dll=dll)
    g, merged = _host_merge(graph, matches, thr_len, solve, dll, **stand_ins)
    if close is None:
        return _host_tail(g, merged, dll, detach=detach, rc=rc)
    return _list_tail(g, merged, close, dll, detach=detach, rc=rc)
