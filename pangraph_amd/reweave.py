"""The front half of reweave (packages/pangraph/src/pangraph/reweave.rs:132-340, 408-443): `pga_plan_merge` (include/pga_align.h) turns the
filtered matches of a tree level into new block ids, anchor decisions, the refined interval table of every block with a hit (what
`pga_slice_blocks` takes) and the merge promises with their CIGARs (what `pga_solve_promises` takes).  ctypes only; the HIP library does the
work.  `promise_args` is the pointer arithmetic from this output to `promise.promise_t`."""
import ctypes as C

from . import batch
from .promise import promise_t
from .slice import slice_interval_t

KINDS = "MIDNSHP=XB"


class plan_block_t(C.Structure):
    _fields_ = [("block_id", C.c_uint64), ("consensus", C.c_char_p), ("cons_len", C.c_uint32), ("depth", C.c_uint32)]


class plan_match_t(C.Structure):
    _fields_ = [("new_block_id", C.c_uint64), ("anchor", C.c_int32), ("route", C.c_int32), ("ref_n", C.c_uint32), ("qry_n", C.c_uint32)]


class plan_block_res_t(C.Structure):
    _fields_ = [("first_interval", C.c_uint64), ("fail_interval", C.c_int64), ("block", C.c_uint32), ("n_intervals", C.c_uint32),
                ("status", C.c_int32), ("pad", C.c_int32)]


class plan_interval_t(C.Structure):
    _fields_ = [("new_block_id", C.c_uint64), ("match", C.c_int64), ("start", C.c_uint32), ("end", C.c_uint32), ("aligned", C.c_int32),
                ("is_anchor", C.c_int32), ("reverse", C.c_int32), ("extend_left", C.c_uint32), ("extend_right", C.c_uint32), ("pad", C.c_uint32)]


class plan_promise_t(C.Structure):
    _fields_ = [("new_block_id", C.c_uint64), ("match", C.c_int64), ("anchor_interval", C.c_uint64), ("append_interval", C.c_uint64),
                ("cigar_off", C.c_uint64), ("anchor_block", C.c_uint32), ("append_block", C.c_uint32), ("n_cigar", C.c_uint32), ("reverse", C.c_int32)]


class plan_counters_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("by_depth", "by_mask", "by_letters", "hits", "intervals_before", "intervals_after", "cigar_in", "cigar_out")]


class plan_out_t(C.Structure):
    _fields_ = [("n_matches", C.c_int64), ("n_blocks", C.c_int64), ("n_intervals", C.c_int64), ("n_promises", C.c_int64), ("n_failed", C.c_int64),
                ("n_cigar", C.c_uint64), ("matches", C.POINTER(plan_match_t)), ("blocks", C.POINTER(plan_block_res_t)),
                ("intervals", C.POINTER(plan_interval_t)), ("slice_intervals", C.POINTER(slice_interval_t)), ("promises", C.POINTER(plan_promise_t)),
                ("cigars", C.POINTER(C.c_uint32)), ("counters", plan_counters_t)]


def _bind(dll):
    dll.pga_plan_merge.restype = C.c_int
    dll.pga_plan_merge.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                   C.POINTER(plan_out_t)]
    dll.pga_plan_free.restype = None
    dll.pga_plan_free.argtypes = [C.POINTER(plan_out_t)]
    dll.pga_last_error.restype = C.c_char_p


def pack_cigar(ops):
    """[(kind, len)] -> minimap2 words"""
    return [ln << 4 | KINDS.index(k) for k, ln in ops]


class _Packed:
    """the C arrays of a level: groups of blocks and their matches; keeps every buffer alive"""

    def __init__(self, groups, matches):
        flat = [b for g in groups for b in g]
        off = [0]
        for g in groups:
            off.append(off[-1] + len(g))
        self.n_groups, self.n_blocks, self.n_matches = len(groups), len(flat), len(matches)
        self.off = (C.c_int64 * (len(groups) + 1))(*off)
        self.cons = [None if b["consensus"] is None else b["consensus"] if isinstance(b["consensus"], bytes) else b["consensus"].encode("latin-1") for b in flat]
        self.B = (plan_block_t * max(len(flat), 1))()
        for i, (b, c) in enumerate(zip(flat, self.cons)):
            self.B[i].block_id = b["block_id"]; self.B[i].consensus = c; self.B[i].depth = b["depth"]
            self.B[i].cons_len = b.get("cons_len", len(c) if c is not None else 0)
        self.M = (batch.pga_match_t * max(len(matches), 1))()
        words = []
        for i, m in enumerate(matches):
            r = self.M[i]
            r.group, r.qry, r.ref = m["group"], m["qry"], m["ref"]
            r.qry_start, r.qry_end, r.ref_start, r.ref_end = m["qry_start"], m["qry_end"], m["ref_start"], m["ref_end"]
            r.reverse = 1 if m["reverse"] else 0
            cg = m["cigar"] if not m["cigar"] or isinstance(m["cigar"][0], int) else pack_cigar(m["cigar"])
            r.cigar_off, r.n_cigar = m.get("cigar_off", len(words)), m.get("n_cigar", len(cg))
            words += cg
        self.n_ops = len(words)
        self.G = (C.c_uint32 * max(len(words), 1))(*words)

    def args(self):
        return (self.n_groups, self.off, self.B, self.n_matches, self.M, self.G, self.n_ops)


class PlanOut:
    """the output of one call; lives until free()"""

    def __init__(self, dll, out, keep):
        self.dll, self.out, self.keep = dll, out, keep

    def to_lists(self):
        """-> {"matches", "blocks", "intervals", "slice_intervals", "promises", "cigars", "n_failed", "counters"} as plain lists of dicts
        (intervals, slice_intervals, promises and cigars None when a block failed); a promise carries its CIGAR as [(kind, len)] too"""
        o = self.out
        rec = lambda r, names: {n: getattr(r, n) for n in names}
        res = {"matches": [rec(o.matches[i], ("new_block_id", "anchor", "route", "ref_n", "qry_n")) for i in range(o.n_matches)],
               "blocks": [rec(o.blocks[i], ("block", "n_intervals", "first_interval", "status", "fail_interval")) for i in range(o.n_blocks)],
               "n_failed": o.n_failed, "counters": rec(o.counters, [n for n, _ in plan_counters_t._fields_]),
               "intervals": None, "slice_intervals": None, "promises": None, "cigars": None}
        if not o.n_failed:
            res["intervals"] = [rec(o.intervals[i], ("start", "end", "aligned", "new_block_id", "is_anchor", "reverse", "match", "extend_left", "extend_right"))
                                for i in range(o.n_intervals)]
            res["slice_intervals"] = [(o.slice_intervals[i].start, o.slice_intervals[i].end, o.slice_intervals[i].flip) for i in range(o.n_intervals)]
            res["cigars"] = [o.cigars[i] for i in range(o.n_cigar)]
            res["promises"] = []
            for i in range(o.n_promises):
                p = rec(o.promises[i], ("new_block_id", "match", "reverse", "anchor_block", "anchor_interval", "append_block", "append_interval", "cigar_off", "n_cigar"))
                p["cigar"] = [(KINDS[w & 15], w >> 4) for w in res["cigars"][p["cigar_off"]:p["cigar_off"] + p["n_cigar"]]]
                res["promises"].append(p)
        return res

    def free(self):
        if self.out is not None:
            self.dll.pga_plan_free(C.byref(self.out))
            self.out = None


def plan_merge_raw(args, thr_len, batch_handle=None, seq_index=None, dll=None, keep=None):
    """args: (n_groups, group_off, blocks, n_matches, matches, cigars, n_ops) as C arrays or pointers (a _Packed's args(), or the arrays of a
    filtered result); batch_handle: a ResidentBatch's handle with seq_index (an int64 array, one entry per block) -> PlanOut"""
    dll = dll or batch.lib()
    _bind(dll)
    out = plan_out_t()
    if dll.pga_plan_merge(*args, thr_len, batch_handle, seq_index, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return PlanOut(dll, out, (keep, seq_index))


def plan_merge(groups, matches, thr_len, batch=None, seq_index=None, dll=None):
    """groups: [[{"block_id", "consensus", "depth"}]] (the blocks of every merge of a tree level); matches: [{"group", "qry", "ref" (indices
    inside the group), "qry_start", "qry_end", "ref_start", "ref_end", "reverse", "cigar": [(kind, len)] or packed words}]; batch: the
    ResidentBatch the blocks lie in, block i being its sequence seq_index[i] (default: i) -> PlanOut.to_lists()"""
    K = _Packed(groups, matches)
    handle = idx = None
    if batch is not None:
        seq_index = list(range(K.n_blocks)) if seq_index is None else list(seq_index)
        idx = (C.c_int64 * max(len(seq_index), 1))(*seq_index)
        handle = batch.h
    out = plan_merge_raw(K.args(), thr_len, handle, idx, dll, keep=K)
    try:
        return out.to_lists()
    finally:
        out.free()


def promise_args(plan, blocks):
    """plan: a PlanOut (alive); blocks: the plan_block_t array the call was given -> a promise_t array with everything but n_members filled
    in by pointer arithmetic: consensus + start, end - start, cigars + cigar_off (the members of promise p are the kept members of the append
    slice, pga_slice_blocks' counts)"""
    o = plan.out
    P = (promise_t * max(o.n_promises, 1))()
    base = lambda i: C.c_void_p.from_address(C.addressof(blocks[i]) + plan_block_t.consensus.offset).value or 0
    cig = C.addressof(o.cigars.contents) if o.n_promises else 0
    for p in range(o.n_promises):
        r = o.promises[p]
        a, q = o.intervals[r.anchor_interval], o.intervals[r.append_interval]
        C.c_void_p.from_address(C.addressof(P[p]) + promise_t.anchor.offset).value = base(r.anchor_block) + a.start
        C.c_void_p.from_address(C.addressof(P[p]) + promise_t.append.offset).value = base(r.append_block) + q.start
        P[p].anchor_len, P[p].append_len, P[p].reverse = a.end - a.start, q.end - q.start, r.reverse
        C.c_void_p.from_address(C.addressof(P[p]) + promise_t.cigar.offset).value = cig + 4 * r.cigar_off
        P[p].n_cigar = r.n_cigar
    return P


# ---------------------------------------------------------------- the graph level: host bookkeeping over ids and paths
class ReweaveError(Exception):
    """the reference's reweave returns Err: a block fails refine_intervals (its status and interval are in the message)"""


def _apply_update(g, p, bids, order, sliced_in, rows, update, dll):
    """the graph update behind the slices as one pga_apply_merge call (update == "device") or a stand-in for it (a callable: blocks, paths,
    nodes, cut, intervals, slices, members as lists -> what apply.ApplyOut.to_lists() gives), read back into the dicts -> halves"""
    from . import apply as ap, topology as tp
    args = tp.pack_graph(g, {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()})
    at = {b: i for i, b in enumerate(sorted(g["blocks"]))}
    cut = [(at[bids[b["block"]]], b["n_intervals"], b["first_interval"]) for b in p["blocks"]]
    slices, members = [], []
    for per_iv in rows:
        for r in per_iv:
            slices.append((len(members), len(r["kept"]), len(r["dropped"])))
            members += [(m["member"], m["reverse"], m["pos"][0], m["pos"][1]) for m in r["kept"]]
    if update == "device":
        K = ap.pack_cut_lists(cut, p["intervals"], slices, members)
        out = ap.apply_merge_raw(args, *K, dll=dll, keep=(args, K))
        try:
            res = out.to_lists(args[0])
        finally:
            out.free()
    else:
        res = update(*tp.unpack_lists(args), cut, p["intervals"], slices, members)
    old = {n: g["nodes"].pop(n) for nids in order for n in nids}
    halves, k = {}, 0
    for b, blk, per_iv in zip(p["blocks"], sliced_in, rows):
        for j, r in enumerate(per_iv):
            iv = p["intervals"][b["first_interval"] + j]
            new_block = {"consensus": blk["consensus"][iv["start"]:iv["end"]], "alignments": {}}
            for m in r["kept"]:
                nid, pos0, pos1, _, _, rev = res["new_nodes"][k]
                new_block["alignments"][nid] = {"subs": list(m["subs"]), "dels": list(m["dels"]), "inss": list(m["inss"])}
                g["nodes"][nid] = {"block_id": iv["new_block_id"], "path_id": old[res["old_node"][k]]["path_id"], "strand": "-" if rev else "+", "position": (pos0, pos1)}
                k += 1
            if iv["aligned"]:
                halves[(iv["new_block_id"], bool(iv["is_anchor"]))] = new_block
            else:
                g["blocks"][iv["new_block_id"]] = new_block
    for b in p["blocks"]:
        del g["blocks"][bids[b["block"]]]
    for pid, off, n, _ in res["paths"]:
        g["paths"][pid]["nodes"] = [x[0] for x in res["nodes"][off:off + n]]
    return halves


def reweave(graph, matches, thr_len, dll=None, plan=None, slicer=None, update=None):
    """reweave (reweave.rs:408-453) on a graph in the shape of simplify.normalize() (changed in place and returned).
    matches: [{"qry": block id, "ref": block id, "qry_start", "qry_end", "ref_start", "ref_end", "reverse", "cigar"}].
    plan -> pga_slice_blocks -> node ids (simplify.node_id) -> GraphUpdate (reweave.rs:359-401, 445-450; a reverse old node gets its new
    nodes in reverse order).  -> (graph, promises): a promise is {"new_block_id", "anchor": block, "append": block, "reverse", "cigar"}
    with block = {"consensus", "alignments": {new node id: edit}} -- what promise.solve_promises takes per promise is (anchor consensus,
    append consensus, reverse, [(len, kind)], the append block's edits in node id order).
    plan / slicer stand in for the device calls (groups, matches, thr_len -> plan_merge's result; blocks -> slice_blocks' result).
    update: None -- the loop over the dicts below; "device" -- one pga_apply_merge call (pangraph_amd/apply.py) on topology.pack_graph's arrays,
    read back into the same dicts; a callable stands in for that call."""
    from . import simplify, slice as sl
    g = graph
    bids = sorted({m["qry"] for m in matches} | {m["ref"] for m in matches})
    index = {b: k for k, b in enumerate(bids)}
    blocks = [{"block_id": b, "consensus": g["blocks"][b]["consensus"], "depth": len(g["blocks"][b]["alignments"])} for b in bids]
    ms = [dict(m, group=0, qry=index[m["qry"]], ref=index[m["ref"]]) for m in matches]
    p = (plan or (lambda gr, mt, thr: plan_merge(gr, mt, thr, dll=dll)))([blocks], ms, thr_len)
    if p["n_failed"]:
        bad = [b for b in p["blocks"] if b["status"]][0]
        raise ReweaveError(f"block {bids[bad['block']]}: refine_intervals fails with code {bad['status']} at interval {bad['fail_interval']}")
    order, sliced_in = [], []
    for b in p["blocks"]:
        bid = bids[b["block"]]
        nids = sorted(g["blocks"][bid]["alignments"])
        order.append(nids)
        old = [g["nodes"][n] for n in nids]
        sliced_in.append({"consensus": g["blocks"][bid]["consensus"], "members": [g["blocks"][bid]["alignments"][n] for n in nids],
                          "nodes": [(o["position"][0], o["position"][1], g["paths"][o["path_id"]]["tot_len"], o["strand"] == "-", g["paths"][o["path_id"]]["circular"]) for o in old],
                          "intervals": p["slice_intervals"][b["first_interval"]:b["first_interval"] + b["n_intervals"]]})
    rows = (slicer or (lambda bl: sl.slice_blocks(bl, dll=dll)))(sliced_in)
    if update is not None:
        halves = _apply_update(g, p, bids, order, sliced_in, rows, update, dll)
        return g, [{"new_block_id": q["new_block_id"], "anchor": halves[(q["new_block_id"], True)], "append": halves[(q["new_block_id"], False)],
                    "reverse": bool(q["reverse"]), "cigar": list(q["cigar"])} for q in p["promises"]]
    halves, n_new = {}, {}
    for b, nids, blk, per_iv in zip(p["blocks"], order, sliced_in, rows):
        for n in nids:
            n_new[n] = []
        for k, r in enumerate(per_iv):
            iv = p["intervals"][b["first_interval"] + k]
            new_block = {"consensus": blk["consensus"][iv["start"]:iv["end"]], "alignments": {}}
            for m in r["kept"]:
                old_id = nids[m["member"]]
                path = g["nodes"][old_id]["path_id"]
                nid = simplify.node_id(iv["new_block_id"], path, m["reverse"], m["pos"])
                new_block["alignments"][nid] = {"subs": list(m["subs"]), "dels": list(m["dels"]), "inss": list(m["inss"])}
                n_new[old_id].append((nid, {"block_id": iv["new_block_id"], "path_id": path, "strand": "-" if m["reverse"] else "+", "position": tuple(m["pos"])}))
            if iv["aligned"]:
                halves[(iv["new_block_id"], bool(iv["is_anchor"]))] = new_block
            else:
                g["blocks"][iv["new_block_id"]] = new_block
    for b in p["blocks"]:
        del g["blocks"][bids[b["block"]]]
    for old_id, new in n_new.items():
        old = g["nodes"].pop(old_id)
        if old["strand"] == "-":
            new.reverse()
        for nid, node in new:
            g["nodes"][nid] = node
        nodes = g["paths"][old["path_id"]]["nodes"]
        at = nodes.index(old_id)
        nodes[at:at + 1] = [nid for nid, _ in new]
    promises = [{"new_block_id": q["new_block_id"], "anchor": halves[(q["new_block_id"], True)], "append": halves[(q["new_block_id"], False)],
                 "reverse": bool(q["reverse"]), "cigar": list(q["cigar"])} for q in p["promises"]]
    return g, promises
