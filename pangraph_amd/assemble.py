"""The block arrays behind a merge round on the device: `pga_assemble_blocks` (include/pga_align.h, pga_assemble.hip) executes the gather list
of pga_apply_merge -- the consensus pointers, member counts, three edit lists and insertion letters of every block of the graph after, from
the outputs of pga_plan_merge, pga_slice_blocks, pga_solve_promises and pga_apply_merge as they stand: solve_promise's tail (reweave.rs:88-93),
the insertion of the merged blocks (graph_merging.rs:156-165) and the blocks split_block leaves (reweave.rs:359-401) in one call.  ctypes and
numpy only; the HIP library does the work.

An output's `block_args()` are the first seven arguments of pga_detach_unaligned, pga_reconsensus, pga_reconstruct, pga_merge_blocks,
pga_remove_paths (rc side) and the exports, its `who` the who argument of pga_detach_unaligned: pointers, nothing is copied.
`detach.merged_blocks` is the same gather for the merged blocks alone, in numpy on the host."""
import ctypes as C

import numpy as np

from . import batch
from .apply import apply_block_t, apply_cut_t, apply_out_t
from .detach import DEL, INS, SUB, detach_member_t
from .mapvar import del_t, ins_t, res_t, sub_t
from .reconsensus import rc_block_t, rc_member_t
from .remove import edits_to_dicts
from .reweave import plan_interval_t, plan_promise_t
from .slice import slice_member_t, slice_out_t, slice_res_t
from .topology import topo_block_t, topo_node_t

MERGED_ONLY = 1                      # PGA_ASSEMBLE_MERGED_ONLY
TILE = 1024                          # PGA_ASSEMBLE_TILE
NONE = 0xFFFFFFFF


class assemble_out_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int64), ("n_members", C.c_int64), ("n_subs", C.c_uint64), ("n_dels", C.c_uint64), ("n_inss", C.c_uint64),
                ("n_ins_letters", C.c_uint64), ("blocks", C.POINTER(rc_block_t)), ("members", C.POINTER(rc_member_t)), ("subs", C.POINTER(sub_t)),
                ("dels", C.POINTER(del_t)), ("inss", C.POINTER(ins_t)), ("ins_seq", C.POINTER(C.c_char)), ("who", C.POINTER(detach_member_t)),
                ("origin", C.POINTER(C.c_int64))]


def _bind(dll):
    dll.pga_assemble_blocks.restype = C.c_int
    dll.pga_assemble_blocks.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p] + \
        [C.c_void_p] * 5 + [C.c_uint64, C.c_void_p, C.c_uint32, C.POINTER(assemble_out_t)]
    dll.pga_assemble_free.restype = None
    dll.pga_assemble_free.argtypes = [C.POINTER(assemble_out_t)]
    dll.pga_assemble_last_ms.restype = None
    dll.pga_assemble_last_ms.argtypes = [C.POINTER(C.c_double)]
    dll.pga_last_error.restype = C.c_char_p


def _ptr(p):
    if p is None or isinstance(p, int):
        return p
    if isinstance(p, np.ndarray):
        return C.c_void_p(p.ctypes.data) if p.size else None
    if isinstance(p, C.Structure):
        return C.cast(C.pointer(p), C.c_void_p)
    return C.cast(p, C.c_void_p)


def _view(ptr, n, dtype):
    """n records behind a ctypes pointer as a numpy array of their own"""
    if not n:
        return np.zeros(0, dtype)
    return np.frombuffer(C.string_at(ptr, n * dtype.itemsize), dtype).copy()


MEMBER = np.dtype([("n_subs", "<u4"), ("n_dels", "<u4"), ("n_inss", "<u4")])
WHO = np.dtype([("node_id", "<u8"), ("reverse", "<i4"), ("pad", "<i4")])
assert (MEMBER.itemsize, WHO.itemsize) == (C.sizeof(rc_member_t), C.sizeof(detach_member_t))


# ---------------------------------------------------------------- the call
class AssembleOut:
    """the output of one call; owns its arrays until free().  `block_args()` are pointers into this output: the consensus pointers lead into
    the caller's consensus letters, everything else is the call's own."""

    def __init__(self, dll, out, keep):
        self.dll, self.out, self.keep = dll, out, keep

    def block_args(self):
        o = self.out
        return (o.n_blocks, _ptr(o.blocks), _ptr(o.members), _ptr(o.subs), _ptr(o.dels), _ptr(o.inss), _ptr(o.ins_seq))

    @property
    def who(self):
        """the detach_member_t array of the output (the who argument of detach.detach_unaligned_raw), or None when no block was cut"""
        o = self.out
        return C.cast(o.who, C.POINTER(detach_member_t * max(o.n_members, 1))).contents if o.who else None

    @property
    def origin(self):
        return self.out.origin[:self.out.n_members] if self.out.n_members else []

    def to_arrays(self):
        """{"blocks": [(consensus, n_members)], "counts" (members, 3), "subs", "dels", "inss", "ins_seq", "who": [(node_id, reverse)] or None, "origin", "totals"}: numpy
        copies of every array (the lists in the record dtypes of pangraph_amd/detach.py)"""
        o = self.out
        blocks = []
        for b in range(o.n_blocks):
            at = C.c_void_p.from_address(C.addressof(o.blocks[b])).value             # (the field is a c_char_p: reading it would stop at a NUL)
            blocks.append((C.string_at(at, o.blocks[b].cons_len) if at and o.blocks[b].cons_len else b"", o.blocks[b].n_members))
        who = _view(o.who, o.n_members, WHO) if o.who else None
        return {"blocks": blocks, "counts": _view(o.members, o.n_members, MEMBER).view(np.uint32).reshape(-1, 3), "subs": _view(o.subs, o.n_subs, SUB), "dels": _view(o.dels, o.n_dels, DEL),
                "inss": _view(o.inss, o.n_inss, INS), "ins_seq": C.string_at(o.ins_seq, o.n_ins_letters) if o.n_ins_letters else b"",
                "who": None if who is None else list(zip(who["node_id"].tolist(), who["reverse"].tolist())), "origin": list(self.origin),
                "totals": (o.n_blocks, o.n_members, o.n_subs, o.n_dels, o.n_inss, o.n_ins_letters)}

    def to_dicts(self):
        """per output block {"consensus", "members": [edit]} (remove.edits_to_dicts)"""
        return edits_to_dicts(*self.block_args())

    def free(self):
        if self.out is not None:
            self.dll.pga_assemble_free(C.byref(self.out))
            self.out = None


def plan_args(plan, n_cut, cut):
    """plan: a reweave.PlanOut (alive); (n_cut, cut): apply.pack_cut's -> the `plan` argument of assemble_blocks_raw"""
    o = plan.out
    return (n_cut, cut, o.intervals, o.n_promises, o.promises)


def promise_args(raw):
    """raw: what promise.solve_promises_raw returns -> the `promise_out` argument of assemble_blocks_raw (the letters of the results are packed,
    so their count is the sum of n_ins_bases)"""
    K, R, subs, dels, inss, iseq = raw[:6]
    return (R, subs, dels, inss, iseq, sum(R[m].n_ins_bases for m in range(K.n_mem)))


def assemble_blocks_raw(block_args, plan, slice_out, promise_out, apply_out, flags=0, dll=None, keep=None, ins_seq_len=None):
    """block_args: (n_blocks, rc_blocks, members, subs, dels, inss, ins_seq) of the graph BEFORE as C arrays, numpy arrays or pointers (a
    reconstruct._Packed's args()[:7], remove.pack_blocks, the block_args() of an earlier output), ins_seq_len its letter count (default: the
    size of a ctypes buffer); plan: (n_cut, cut, intervals, n_promises, promises) (plan_args); slice_out: the slice_out_t of
    slice.slice_blocks_raw; promise_out: (res, subs, dels, inss, ins_seq, ins_seq_len) (promise_args) or None; apply_out: an apply.ApplyOut or
    its apply_out_t -> AssembleOut"""
    dll = dll or batch.lib()
    _bind(dll)
    if ins_seq_len is None:
        ins_seq_len = C.sizeof(block_args[6]) if isinstance(block_args[6], C.Array) else len(block_args[6]) if isinstance(block_args[6], (bytes, bytearray)) else 0
    n_cut, cut, intervals, n_promises, promises = plan
    res, p_subs, p_dels, p_inss, p_seq, p_len = promise_out or (None, None, None, None, None, 0)
    applied = getattr(apply_out, "out", apply_out)
    out = assemble_out_t()
    if dll.pga_assemble_blocks(block_args[0], *[_ptr(a) for a in block_args[1:7]], ins_seq_len, n_cut, _ptr(cut), _ptr(intervals), n_promises, _ptr(promises),
                               _ptr(slice_out), _ptr(res), _ptr(p_subs), _ptr(p_dels), _ptr(p_inss), _ptr(p_seq), p_len, _ptr(applied), flags, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return AssembleOut(dll, out, (keep, block_args, plan, slice_out, promise_out, apply_out))


def last_ms(dll=None):
    """(upload, kernels, download) of the calling thread's last call, in ms on the stream's clock (measurement only)"""
    dll = dll or batch.lib()
    _bind(dll)
    ms = (C.c_double * 3)()
    dll.pga_assemble_last_ms(ms)
    return tuple(ms)


# ---------------------------------------------------------------- the list level
def _records(rows, dtype):
    a = rows if isinstance(rows, np.ndarray) else np.array([tuple(r) for r in rows], dtype) if len(rows) else np.zeros(0, dtype)
    return np.ascontiguousarray(a, dtype)


SLICE_MEMBER = np.dtype([("member", "<u4"), ("reverse", "<i4"), ("node_start", "<u4"), ("node_end", "<u4"), ("pos_start", "<u8"), ("pos_end", "<u8"),
                         ("n_subs", "<u4"), ("n_dels", "<u4"), ("n_inss", "<u4"), ("pad", "<u4"), ("sub_off", "<u8"), ("del_off", "<u8"), ("ins_off", "<u8")])
RES = np.dtype([("status", "<i4"), ("score", "<i4"), ("attempts", "<i4"), ("hit_boundary", "<i4"), ("n_subs", "<u4"), ("n_dels", "<u4"), ("n_inss", "<u4"),
                ("n_ins_bases", "<u4"), ("sub_off", "<u8"), ("del_off", "<u8"), ("ins_off", "<u8")])
assert (SLICE_MEMBER.itemsize, RES.itemsize) == (C.sizeof(slice_member_t), C.sizeof(res_t)) and SLICE_MEMBER.fields["sub_off"][1] == slice_member_t.sub_off.offset


class Tables:
    """the C view of one call's input given as lists and numpy arrays; keeps every buffer alive.  t:
      "blocks": [(consensus bytes, n_members)] of the graph before, "counts": (members, 3), "subs" / "dels" / "inss": SUB / DEL / INS records, "ins_seq": bytes;
      "cut": [(block, n_intervals, first_interval)], "intervals": [{"new_block_id", "start", "end", "aligned", "is_anchor"}], "promises": [(anchor_interval, append_interval)];
      "slices": [(member_off, n_kept, n_dropped)], "s_members": [(n_subs, n_dels, n_inss, sub_off, del_off, ins_off)], "s_subs" / "s_dels" / "s_inss";
      "res": [(status, n_subs, n_dels, n_inss, sub_off, del_off, ins_off)], "p_subs" / "p_dels" / "p_inss", "p_ins_seq": bytes;
      "applied": {"blocks": [(block_id, cons_len, depth, alive)], "nodes": [(node_id, pos0, pos1, block, member, reverse)], "new_blocks", "member_src",
                  "block_map"} as apply.ApplyOut.to_lists() gives them, or None (no cut)."""

    def __init__(self, t):
        nb = len(t["blocks"])
        self.cons = [bytes(c) for c, _ in t["blocks"]]
        self.B = (rc_block_t * max(nb, 1))()
        for i, (c, n) in enumerate(t["blocks"]):
            self.B[i].consensus = self.cons[i]; self.B[i].cons_len = len(self.cons[i]); self.B[i].n_members = n
        self.n_blocks = nb
        self.M = np.ascontiguousarray(np.asarray(t["counts"], np.uint32).reshape(-1, 3))
        self.S, self.D, self.I = _records(t["subs"], SUB), _records(t["dels"], DEL), _records(t["inss"], INS)
        self.L = bytes(t["ins_seq"])
        cut, ivs = t.get("cut", []), t.get("intervals", [])
        self.n_cut = len(cut)
        self.K = (apply_cut_t * max(len(cut), 1))(*[apply_cut_t(*c) for c in cut])
        self.V = (plan_interval_t * max(len(ivs), 1))()
        for r, iv in zip(self.V, ivs):
            r.new_block_id, r.start, r.end, r.aligned, r.is_anchor, r.match = iv["new_block_id"], iv["start"], iv["end"], 1 if iv["aligned"] else 0, 1 if iv["is_anchor"] else 0, -1
        pr = t.get("promises", [])
        self.n_promises = len(pr)
        self.P = (plan_promise_t * max(len(pr), 1))()
        for r, (a, q) in zip(self.P, pr):
            r.anchor_interval, r.append_interval, r.new_block_id = a, q, ivs[a]["new_block_id"] if a < len(ivs) else 0
        sl = t.get("slices", [])
        self.SL = (slice_res_t * max(len(sl), 1))(*[slice_res_t(*s) for s in sl])
        sm = t.get("s_members", [])
        self.SM = np.zeros(len(sm), SLICE_MEMBER)
        if len(sm):
            cols = np.asarray(sm, np.uint64).reshape(-1, 6)
            for k, name in enumerate(("n_subs", "n_dels", "n_inss", "sub_off", "del_off", "ins_off")):
                self.SM[name] = cols[:, k]
        self.SS, self.SD, self.SI = _records(t.get("s_subs", []), SUB), _records(t.get("s_dels", []), DEL), _records(t.get("s_inss", []), INS)
        self.slice = slice_out_t()
        self.slice.slices = C.cast(self.SL, C.POINTER(slice_res_t))
        for name, a, ct in (("members", self.SM, slice_member_t), ("subs", self.SS, sub_t), ("dels", self.SD, del_t), ("inss", self.SI, ins_t)):
            if a.size:
                setattr(self.slice, name, C.cast(C.c_void_p(a.ctypes.data), C.POINTER(ct)))
        rs = t.get("res", [])
        self.R = np.zeros(len(rs), RES)
        if len(rs):
            cols = np.asarray(rs, np.int64).reshape(-1, 7)
            for k, name in enumerate(("status", "n_subs", "n_dels", "n_inss", "sub_off", "del_off", "ins_off")):
                self.R[name] = cols[:, k]
        self.PS, self.PD, self.PI = _records(t.get("p_subs", []), SUB), _records(t.get("p_dels", []), DEL), _records(t.get("p_inss", []), INS)
        self.PL = bytes(t.get("p_ins_seq", b""))
        self.applied = apply_out_t()
        ap = t.get("applied")
        if ap is not None:
            self.AB = (topo_block_t * max(len(ap["blocks"]), 1))(*[topo_block_t(b[0], b[1], b[2], b[3], 0) for b in ap["blocks"]])
            self.AN = np.zeros(len(ap["nodes"]), np.dtype([("node_id", "<u8"), ("pos0", "<u8"), ("pos1", "<u8"), ("block", "<u4"), ("member", "<u4"), ("reverse", "<i4"), ("pad", "<i4")]))
            if len(ap["nodes"]):
                cols = np.array(ap["nodes"], np.uint64).reshape(-1, 6)
                for k, name in enumerate(("node_id", "pos0", "pos1", "block", "member", "reverse")):
                    self.AN[name] = cols[:, k]
            assert self.AN.dtype.itemsize == C.sizeof(topo_node_t)
            self.AE = (apply_block_t * max(len(ap["new_blocks"]), 1))(*[apply_block_t(*e) for e in ap["new_blocks"]])
            self.AS = np.ascontiguousarray(np.asarray(ap["member_src"], np.uint64))
            self.AM = np.ascontiguousarray(np.asarray(ap["block_map"], np.uint32))
            a = self.applied
            a.n_new_nodes, a.n_new_blocks, a.n_blocks, a.n_nodes = len(ap["member_src"]), len(ap["new_blocks"]), len(ap["blocks"]), len(ap["nodes"])
            a.blocks = C.cast(self.AB, C.POINTER(topo_block_t)); a.new_blocks = C.cast(self.AE, C.POINTER(apply_block_t))
            for name, arr, ct in (("nodes", self.AN, topo_node_t), ("member_src", self.AS, C.c_uint64), ("block_map", self.AM, C.c_uint32)):
                if arr.size:
                    setattr(a, name, C.cast(C.c_void_p(arr.ctypes.data), C.POINTER(ct)))

    def block_args(self):
        return (self.n_blocks, self.B, self.M, self.S, self.D, self.I, self.L)

    def call_args(self):
        """(block_args, plan, slice_out, promise_out, apply_out) of assemble_blocks_raw"""
        return (self.block_args(), (self.n_cut, self.K, self.V, self.n_promises, self.P), self.slice, (self.R, self.PS, self.PD, self.PI, self.PL, len(self.PL)), self.applied)


def assemble_blocks(t, flags=0, dll=None):
    """one call on lists (Tables) -> AssembleOut.to_arrays()"""
    K = Tables(t)
    out = assemble_blocks_raw(*K.call_args(), flags=flags, dll=dll, keep=K, ins_seq_len=len(K.L))
    try:
        return out.to_arrays()
    finally:
        out.free()


# ---------------------------------------------------------------- the graph level: one merge round (graph_merging.rs:141-165 without the detach)
class MergeError(Exception):
    """the reference's solve_promise returns Err: a member of an append block could not be re-aligned (its status is in the message)"""


def _host_round(g, matches, thr_len, solve, dll, **stand_ins):
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
    return g


class _SliceInput:
    """the arguments of pga_slice_blocks for the cut blocks of a graph whose block arrays are K (a reconstruct._Packed over all blocks): the
    members and lists of the cut blocks gathered block after block -- an insertion keeps its seq_off into K.L, so the sliced edits and the
    survivors share one letter buffer --, the interval table by pointer from the plan"""

    def __init__(self, g, K, order, bids, cut_blocks, plan):
        from .slice import slice_block_t, slice_node_t
        counts = np.frombuffer(K.M, MEMBER)[:K.n_mem].view(np.uint32).reshape(-1, 3).astype(np.int64)
        off = np.zeros((K.n_mem + 1, 3), np.int64)
        off[1:] = np.cumsum(counts, axis=0)
        spans = [(K.mem_first[i], K.mem_first[i + 1]) for i in cut_blocks]
        take = lambda arr, dt, col: np.ascontiguousarray(np.concatenate([np.frombuffer(arr, dt)[off[a, col]:off[b, col]] for a, b in spans])) if spans else np.zeros(0, dt)
        self.M = np.ascontiguousarray(np.concatenate([np.frombuffer(K.M, MEMBER)[a:b] for a, b in spans])) if spans else np.zeros(0, MEMBER)
        self.S, self.D, self.I = take(K.S, SUB, 0), take(K.D, DEL, 1), take(K.I, INS, 2)
        self.n = len(cut_blocks)
        self.B = (slice_block_t * max(self.n, 1))()
        self.N = (slice_node_t * max(len(self.M), 1))()
        m = 0
        for j, i in enumerate(cut_blocks):
            self.B[j].consensus = K.cons[i]; self.B[j].cons_len = len(K.cons[i]); self.B[j].n_members = len(order[bids[i]]); self.B[j].n_intervals = plan.out.blocks[j].n_intervals
            for nid in order[bids[i]]:
                o = g["nodes"][nid]
                path = g["paths"][o["path_id"]]
                self.N[m].pos_start, self.N[m].pos_end, self.N[m].path_len = o["position"][0], o["position"][1], path["tot_len"]
                self.N[m].reverse, self.N[m].circular = int(o["strand"] == "-"), int(bool(path["circular"]))
                m += 1
        self.V = plan.out.slice_intervals

    def args(self):
        return (self.n, _ptr(self.B), _ptr(self.V), _ptr(self.M), _ptr(self.N), _ptr(self.S), _ptr(self.D), _ptr(self.I))


class _PromiseInput:
    """the arguments of pga_solve_promises for the promises of a plan: consensus pointers and CIGARs by pointer arithmetic
    (reweave.promise_args), the kept members of every append slice with their sliced lists gathered promise after promise"""

    def __init__(self, plan, plan_blocks, slice_out):
        from .reweave import promise_args as pointer_args
        o = plan.out
        self.n = o.n_promises
        self.P = pointer_args(plan, plan_blocks)
        M, S, D, I = [], [], [], []
        grab = lambda ptr, first, n, dt: np.frombuffer(C.string_at(C.addressof(ptr.contents) + first * dt.itemsize, n * dt.itemsize), dt) if n else np.zeros(0, dt)
        for p in range(self.n):
            r = slice_out.slices[o.promises[p].append_interval]
            self.P[p].n_members = r.n_kept
            if not r.n_kept:
                continue
            counts = grab(slice_out.counts, r.member_off, r.n_kept, MEMBER)
            first = slice_out.members[r.member_off]
            M.append(counts)
            S.append(grab(slice_out.subs, first.sub_off, int(counts["n_subs"].sum()), SUB)); D.append(grab(slice_out.dels, first.del_off, int(counts["n_dels"].sum()), DEL))
            I.append(grab(slice_out.inss, first.ins_off, int(counts["n_inss"].sum()), INS))
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros(0, dt)
        self.M, self.S, self.D, self.I = cat(M, MEMBER), cat(S, SUB), cat(D, DEL), cat(I, INS)
        self.n_mem = len(self.M)


def _device_round(g, matches, thr_len, dll, params=None, tap=None):
    """tap: called with (block arrays before, graph arrays before, AssembleOut, ApplyOut) while all of them are alive (tests hand them on by pointer)"""
    import contextlib

    from . import apply as ap, mapvar, remove as rm, reweave as rw, slice as sl, topology as tp
    dll = dll or batch.lib()
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    bids = sorted(g["blocks"])
    at = {b: i for i, b in enumerate(bids)}
    graph_args = tp.pack_graph(g, order)
    K = rm.pack_blocks(g, order)
    hit = sorted({m["qry"] for m in matches} | {m["ref"] for m in matches})
    index = {b: k for k, b in enumerate(hit)}
    P = rw._Packed([[{"block_id": b, "consensus": g["blocks"][b]["consensus"], "depth": len(order[b])} for b in hit]],
                   [dict(m, group=0, qry=index[m["qry"]], ref=index[m["ref"]]) for m in matches])
    with contextlib.ExitStack() as stack:
        plan = rw.plan_merge_raw(P.args(), thr_len, dll=dll, keep=P)
        stack.callback(plan.free)
        if plan.out.n_failed:
            bad = [plan.out.blocks[i] for i in range(plan.out.n_blocks) if plan.out.blocks[i].status][0]
            raise rw.ReweaveError(f"block {hit[bad.block]}: refine_intervals fails with code {bad.status} at interval {bad.fail_interval}")
        n_cut, cut = ap.pack_cut(plan, [at[b] for b in hit])
        if n_cut == 0:
            return g
        S = _SliceInput(g, K, order, bids, [cut[c].block for c in range(n_cut)], plan)
        sl._bind(dll)
        slice_out = sl.slice_out_t()
        if dll.pga_slice_blocks(*S.args(), C.byref(slice_out)) != 0:
            raise batch.PgaError(dll.pga_last_error().decode())
        stack.callback(lambda: dll.pga_slice_free(C.byref(slice_out)))
        applied = ap.apply_merge_raw(graph_args, n_cut, cut, plan.out.intervals, slice_out.slices, slice_out.members, dll=dll)
        stack.callback(applied.free)
        Q = _PromiseInput(plan, P.B, slice_out)
        R = (res_t * max(Q.n_mem, 1))()
        subs, dels, inss, iseq = C.POINTER(sub_t)(), C.POINTER(del_t)(), C.POINTER(ins_t)(), C.POINTER(C.c_char)()
        dll.pga_solve_promises.restype = C.c_int
        dll.pga_solve_promises.argtypes = [C.c_int64] + [C.c_void_p] * 8 + [C.POINTER(C.POINTER(sub_t)), C.POINTER(C.POINTER(del_t)), C.POINTER(C.POINTER(ins_t)), C.POINTER(C.POINTER(C.c_char))]
        dll.pga_free.argtypes = [C.c_void_p]
        prm = params or mapvar.params()
        if dll.pga_solve_promises(Q.n, _ptr(Q.P), _ptr(Q.M), _ptr(Q.S), _ptr(Q.D), _ptr(Q.I), _ptr(K.L), C.cast(C.pointer(prm), C.c_void_p), _ptr(R),
                                  C.byref(subs), C.byref(dels), C.byref(inss), C.byref(iseq)) != 0:
            raise batch.PgaError(dll.pga_last_error().decode())
        stack.callback(lambda: [dll.pga_free(C.cast(x, C.c_void_p)) for x in (subs, dels, inss, iseq) if x])
        n_letters = sum(R[m].n_ins_bases for m in range(Q.n_mem))
        try:
            out = assemble_blocks_raw(K.args()[:7], plan_args(plan, n_cut, cut), slice_out, (R, subs, dels, inss, iseq, n_letters), applied, dll=dll, ins_seq_len=C.sizeof(K.L))
        except batch.PgaError as e:
            if "status other than 0" in str(e):
                raise MergeError(str(e)) from None
            raise
        stack.callback(out.free)
        lists = tp.unpack_lists(applied.graph_args())
        if tap is not None:
            tap(K, graph_args, out, applied)
        return rm.graph_after(g, [b[0] for b in lists[0]], lists, out.to_dicts())


def _edits_of(a):
    """an arrays dict (AssembleOut.to_arrays) -> per block {"consensus", "members": [edit]}"""
    res, m, off = [], 0, [0, 0, 0]
    letters = a["ins_seq"]
    for cons, n in a["blocks"]:
        members = []
        for _ in range(n):
            c = [int(x) for x in a["counts"][m]]
            members.append({"subs": [(int(x["pos"]), chr(int(x["alt"]) & 255)) for x in a["subs"][off[0]:off[0] + c[0]]],
                            "dels": [(int(x["pos"]), int(x["len"])) for x in a["dels"][off[1]:off[1] + c[1]]],
                            "inss": [(int(x["pos"]), letters[int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])].decode("latin-1")) for x in a["inss"][off[2]:off[2] + c[2]]]})
            off = [off[q] + c[q] for q in range(3)]
            m += 1
        res.append({"consensus": bytes(cons).decode("latin-1"), "members": members})
    return res


class _EditPool:
    """edit dicts flattened into the three record lists and one letter buffer"""

    def __init__(self):
        self.subs, self.dels, self.inss, self.letters = [], [], [], bytearray()

    def add(self, e):
        """-> (n_subs, n_dels, n_inss, sub_off, del_off, ins_off)"""
        row = (len(e["subs"]), len(e["dels"]), len(e["inss"]), len(self.subs), len(self.dels), len(self.inss))
        self.subs += [(pos, ord(a)) for pos, a in e["subs"]]
        self.dels += [tuple(d) for d in e["dels"]]
        for pos, seq in e["inss"]:
            self.inss.append((pos, len(seq), len(self.letters)))
            self.letters += seq.encode("latin-1")
        return row


def _list_round(g, matches, thr_len, solve, blocks, dll, plan=None, slicer=None, update=None):
    """the round on lists: the tables of one pga_assemble_blocks call (Tables) built from the list level of the plan, slice, apply and promise
    entries (or their stand-ins), `blocks(tables, flags)` in place of the call, its arrays read back into the dicts"""
    from . import apply as ap, remove as rm, reweave as rw, slice as sl, topology as tp
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    bids = sorted(g["blocks"])
    at = {b: i for i, b in enumerate(bids)}
    hit = sorted({m["qry"] for m in matches} | {m["ref"] for m in matches})
    index = {b: k for k, b in enumerate(hit)}
    groups = [[{"block_id": b, "consensus": g["blocks"][b]["consensus"], "depth": len(order[b])} for b in hit]]
    p = (plan or (lambda gr, mt, thr: rw.plan_merge(gr, mt, thr, dll=dll)))(groups, [dict(m, group=0, qry=index[m["qry"]], ref=index[m["ref"]]) for m in matches], thr_len)
    if p["n_failed"]:
        bad = [b for b in p["blocks"] if b["status"]][0]
        raise rw.ReweaveError(f"block {hit[bad['block']]}: refine_intervals fails with code {bad['status']} at interval {bad['fail_interval']}")
    if not p["blocks"]:
        return g
    sliced_in = []
    for b in p["blocks"]:
        bid = hit[b["block"]]
        old = [g["nodes"][n] for n in order[bid]]
        sliced_in.append({"consensus": g["blocks"][bid]["consensus"], "members": [g["blocks"][bid]["alignments"][n] for n in order[bid]],
                          "nodes": [(o["position"][0], o["position"][1], g["paths"][o["path_id"]]["tot_len"], o["strand"] == "-", g["paths"][o["path_id"]]["circular"]) for o in old],
                          "intervals": p["slice_intervals"][b["first_interval"]:b["first_interval"] + b["n_intervals"]]})
    rows = (slicer or (lambda bl: sl.slice_blocks(bl, dll=dll)))(sliced_in)
    # ---- the graph before and the sliced edits: one letter buffer
    pool = _EditPool()
    counts = [pool.add(g["blocks"][b]["alignments"][n])[:3] for b in bids for n in order[b]]
    cut = [(at[hit[b["block"]]], b["n_intervals"], b["first_interval"]) for b in p["blocks"]]
    slices, members, s_members, kept_of, first_sliced = [], [], [], [], (len(pool.subs), len(pool.dels), len(pool.inss))
    for per_iv in rows:
        for r in per_iv:
            slices.append((len(members), len(r["kept"]), len(r["dropped"])))
            kept_of.append(r["kept"])
            for m in r["kept"]:
                members.append((m["member"], m["reverse"], m["pos"][0], m["pos"][1]))
                row = pool.add(m)
                s_members.append(row[:3] + tuple(row[3 + q] - first_sliced[q] for q in range(3)))
    graph = tp.unpack_lists(tp.pack_graph(g, order))
    applied = update(*graph, cut, p["intervals"], slices, members) if update is not None else ap.apply_merge(*graph, cut, p["intervals"], slices, members, dll=dll)
    # ---- the promises: the kept members of every append slice, in slice order
    interval_of = {(iv["new_block_id"], bool(iv["is_anchor"])): s for s, iv in enumerate(p["intervals"]) if iv["aligned"]}
    cons_of = lambda s: sliced_in[[k for k, b in enumerate(p["blocks"]) if b["first_interval"] <= s < b["first_interval"] + b["n_intervals"]][0]]["consensus"][p["intervals"][s]["start"]:p["intervals"][s]["end"]]
    pairs = [(interval_of[(q["new_block_id"], True)], interval_of[(q["new_block_id"], False)]) for q in p["promises"]]
    edit = lambda m: {"subs": m["subs"], "dels": m["dels"], "inss": m["inss"]}
    solved = solve([(cons_of(a), cons_of(b), bool(q["reverse"]), [(ln, kind) for kind, ln in q["cigar"]], [edit(m) for m in kept_of[b]]) for q, (a, b) in zip(p["promises"], pairs)])
    results, res = _EditPool(), []
    for q, per in zip(p["promises"], solved):
        for k, r in enumerate(per):
            if r["status"] != 0:
                raise MergeError(f"promise {q['new_block_id']}, member {k}: status {r['status']}")
            res.append((0,) + results.add(r))
    t = {"blocks": [(g["blocks"][b]["consensus"].encode("latin-1"), len(order[b])) for b in bids], "counts": counts,
         "subs": pool.subs[:first_sliced[0]], "dels": pool.dels[:first_sliced[1]], "inss": pool.inss[:first_sliced[2]], "ins_seq": bytes(pool.letters),
         "cut": cut, "intervals": p["intervals"], "promises": pairs, "slices": slices, "s_members": s_members,
         "s_subs": pool.subs[first_sliced[0]:], "s_dels": pool.dels[first_sliced[1]:], "s_inss": pool.inss[first_sliced[2]:],
         "res": res, "p_subs": results.subs, "p_dels": results.dels, "p_inss": results.inss, "p_ins_seq": bytes(results.letters),
         "applied": {k: applied[k] for k in ("blocks", "nodes", "new_blocks", "member_src", "block_map")}}
    arrays = blocks(t, 0)
    lists = (applied["blocks"], applied["paths"], applied["nodes"])
    return rm.graph_after(g, [b[0] for b in lists[0]], lists, _edits_of(arrays))


def merge_round(graph, matches, thr_len, solve=None, blocks=None, dll=None, **stand_ins):
    """One merge round on a graph in the shape of simplify.normalize(): reweave (reweave.rs:408-453), solve_promise for every promise
    (reweave.rs:40-94) and the insertion of the merged blocks (graph_merging.rs:156-165) -- graph_merging.rs:141-165 without the detach.
    matches: as reweave() takes them.  -> the graph after (with blocks=None the one given, changed in place).
    blocks=None: the host reweave(), `solve` (promises as promise.solve_promises takes them -> its result) per promise, and the union of the
    anchor members with the re-aligned append members in dicts; plan= / slicer= stand in for the device calls of reweave().
    blocks="device": the same round chained through pga_plan_merge -> pga_slice_blocks -> pga_apply_merge -> pga_solve_promises ->
    pga_assemble_blocks on one set of arrays (the sliced edits and the survivors share one letter buffer; what the next call takes, it takes
    by pointer), read back into the dicts once at the end.
    blocks=callable: stands in for the pga_assemble_blocks call: `blocks(tables, flags)` gets the input of one call as assemble.Tables takes
    it and returns what AssembleOut.to_arrays() gives; the tables are built from the list level of the other entries (plan= / slicer= /
    update= stand in for those, as in reweave()) and `solve`, and the arrays are read back as the device round reads them.
    A member that cannot be re-aligned raises MergeError in every mode."""
    if blocks is None:
        from .promise import solve_promises
        return _host_round(graph, matches, thr_len, solve or (lambda promises: solve_promises(promises, dll=dll)), dll, **stand_ins)
    if blocks == "device":
        return _device_round(graph, matches, thr_len, dll)
    from .promise import solve_promises
    return _list_round(graph, matches, thr_len, solve or (lambda promises: solve_promises(promises, dll=dll)), blocks, dll, **stand_ins)
