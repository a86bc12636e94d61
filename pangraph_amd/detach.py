"""detach_unaligned_nodes (packages/pangraph/src/pangraph/detach_unaligned.rs:24-114): the members of a batch of blocks that hold no aligned
position leave their blocks and become singleton blocks of their own sequences.  The consensus letters and edit lists are
`pga_detach_unaligned` (include/pga_align.h); the node map, O(orphans), is done here, and so is the tail of solve_promise
(reweave.rs:88-93): `merged_blocks` joins the anchor blocks' members with the output of `pga_solve_promises` into the arrays this entry
takes.  ctypes and numpy only; the HIP library does the work."""
import ctypes as C

import numpy as np

from . import batch
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_block_t, rc_member_t
from .reconstruct import _Packed
from .simplify import _MASK, _PRIME, _rol, normalize  # noqa: F401


class detach_member_t(C.Structure):
    _fields_ = [("node_id", C.c_uint64), ("reverse", C.c_int32), ("pad", C.c_int32)]


class detach_orphan_t(C.Structure):
    _fields_ = [("member", C.c_uint64), ("node_id", C.c_uint64), ("block_id", C.c_uint64), ("block", C.c_uint32), ("len", C.c_uint32),
                ("status", C.c_int32), ("pad", C.c_int32)]


class detach_out_t(C.Structure):
    _fields_ = [("n_blocks", C.c_int64), ("n_orphans", C.c_int64), ("blocks", C.POINTER(rc_block_t)), ("members", C.POINTER(rc_member_t)),
                ("subs", C.POINTER(sub_t)), ("dels", C.POINTER(del_t)), ("inss", C.POINTER(ins_t)), ("cons", C.POINTER(C.c_char)),
                ("member_map", C.POINTER(C.c_int64)), ("orphans", C.POINTER(detach_orphan_t))]


class DetachError(Exception):
    """the reference returns Err (a reverse orphan holds a letter the complement table rejects), or a literal '-' came out"""


def _bind(dll):
    dll.pga_detach_unaligned.restype = C.c_int
    dll.pga_detach_unaligned.argtypes = [C.c_int64] + [C.c_void_p] * 7 + [C.POINTER(detach_out_t)]
    dll.pga_detach_free.restype = None
    dll.pga_detach_free.argtypes = [C.POINTER(detach_out_t)]
    dll.pga_last_error.restype = C.c_char_p


# ---------------------------------------------------------------- id((node_id, &seq)) of utils/id.rs: XXH64, seed 0
def xxh64(data, seed=0):
    """XXH64 of a bytes object (the primes and the rotation are those of simplify.node_id)"""
    p1, p2, p3, p4, p5 = _PRIME
    rnd = lambda acc, w: (_rol((acc + w * p2) & _MASK, 31) * p1) & _MASK
    n, at = len(data), 0
    word = lambda k, size: int.from_bytes(data[k:k + size], "little")
    if n >= 32:
        v = [(seed + p1 + p2) & _MASK, (seed + p2) & _MASK, seed & _MASK, (seed - p1) & _MASK]
        while n - at >= 32:
            v = [rnd(v[i], word(at + 8 * i, 8)) for i in range(4)]
            at += 32
        h = (_rol(v[0], 1) + _rol(v[1], 7) + _rol(v[2], 12) + _rol(v[3], 18)) & _MASK
        for a in v:
            h = ((h ^ rnd(0, a)) * p1 + p4) & _MASK
    else:
        h = (seed + p5) & _MASK
    h = (h + n) & _MASK
    while n - at >= 8:
        h = (_rol(h ^ rnd(0, word(at, 8)), 27) * p1 + p4) & _MASK
        at += 8
    if n - at >= 4:
        h = (_rol(h ^ ((word(at, 4) * p1) & _MASK), 23) * p2 + p3) & _MASK
        at += 4
    while at < n:
        h = (_rol(h ^ ((data[at] * p5) & _MASK), 11) * p1) & _MASK
        at += 1
    h ^= h >> 33
    h = (h * p2) & _MASK
    h ^= h >> 29
    h = (h * p3) & _MASK
    return h ^ (h >> 32)


def block_id_stream(node_id, seq):
    """what the derived Hash of (NodeId(usize), &Seq) writes: the id and the length as little-endian u64, then the letters"""
    seq = seq if isinstance(seq, (bytes, bytearray)) else seq.encode("latin-1")
    return (node_id & _MASK).to_bytes(8, "little") + len(seq).to_bytes(8, "little") + bytes(seq)


def block_id(node_id, seq):
    return xxh64(block_id_stream(node_id, seq))


# ---------------------------------------------------------------- the call
class DetachOut:
    """the output of one call; `graph_args(ins_seq)` are the first seven arguments of pga_reconsensus' member arrays, of the next
    pga_detach_unaligned call or of pga_reconstruct: pointers into this output and the caller's own insertion letters, nothing is copied.
    Lives until free()."""

    def __init__(self, dll, out, n_mem, keep):
        self.dll, self.out, self.n_mem, self.keep = dll, out, n_mem, keep
        self.n_blocks, self.n_orphans = out.n_blocks, out.n_orphans
        self.n_in = self.n_blocks - self.n_orphans

    def graph_args(self, ins_seq):
        o = self.out
        cast = lambda p: C.cast(p, C.c_void_p)
        return (self.n_blocks, cast(o.blocks), cast(o.members), cast(o.subs), cast(o.dels), cast(o.inss), ins_seq)

    def member_map(self):
        return [self.out.member_map[m] for m in range(self.n_mem)]

    def n_members(self):
        return [self.out.blocks[b].n_members for b in range(self.n_blocks)]

    def orphans(self):
        """per orphan {"member", "node_id", "block_id", "block", "len", "status", "seq", "cons_off"} (the letters of an orphan with a
        non-zero status are as built, not to be used)"""
        o, res = self.out, []
        for k in range(self.n_orphans):
            r = o.orphans[k]
            at = C.c_void_p.from_address(C.addressof(o.blocks[r.block])).value      # (the field is a c_char_p: reading it would stop at a NUL)
            res.append({"member": r.member, "node_id": r.node_id, "block_id": r.block_id, "block": r.block, "len": r.len, "status": r.status,
                        "seq": C.string_at(at, r.len).decode("latin-1") if r.len else "", "cons_off": at - C.addressof(o.cons.contents)})
        return res

    def to_dicts(self, ins_seq, with_offsets=False):
        """every output block {"consensus", "members": [edit]}; ins_seq: the caller's insertion letters (a ctypes buffer or bytes)"""
        o = self.out
        base = ins_seq if isinstance(ins_seq, (bytes, bytearray)) else C.string_at(ins_seq, C.sizeof(ins_seq)) if ins_seq is not None else b""
        res, m, s, d, i = [], 0, 0, 0, 0
        for b in range(self.n_blocks):
            blk = o.blocks[b]
            at = C.c_void_p.from_address(C.addressof(blk)).value
            members = []
            for _ in range(blk.n_members):
                c = o.members[m]
                ed = {"subs": [(o.subs[k].pos, chr(o.subs[k].alt & 255)) for k in range(s, s + c.n_subs)], "dels": [(o.dels[k].pos, o.dels[k].len) for k in range(d, d + c.n_dels)],
                      "inss": [(o.inss[k].pos, base[o.inss[k].seq_off:o.inss[k].seq_off + o.inss[k].len].decode("latin-1")) for k in range(i, i + c.n_inss)]}
                if with_offsets:
                    ed["seq_off"] = [o.inss[k].seq_off for k in range(i, i + c.n_inss)]
                s += c.n_subs; d += c.n_dels; i += c.n_inss; m += 1
                members.append(ed)
            res.append({"consensus": C.string_at(at, blk.cons_len).decode("latin-1") if blk.cons_len else "", "members": members})
        assert m == self.n_mem
        return res

    def free(self):
        if self.out is not None:
            self.dll.pga_detach_free(C.byref(self.out))
            self.out = None


def detach_unaligned_raw(graph_args, who, dll=None, keep=None):
    """graph_args: (n_blocks, blocks, members, subs, dels, inss, ins_seq) as C arrays or pointers (a _Packed's args()[:7], arrays_args(), a
    MergeOut's or a DetachOut's graph_args()); who: [(node_id, reverse)] per global member, a detach_member_t array, or None -> DetachOut"""
    dll = dll or batch.lib()
    _bind(dll)
    if who is None or isinstance(who, C.Array):
        W, n_mem = who, (len(who) if who is not None else 0)
    else:
        n_mem = len(who)
        W = (detach_member_t * max(n_mem, 1))(*[detach_member_t(n & _MASK, 1 if rev else 0, 0) for n, rev in who])
    out = detach_out_t()
    if dll.pga_detach_unaligned(*graph_args, W, C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return DetachOut(dll, out, n_mem, (keep, W))


def detach_unaligned(blocks, who, dll=None):
    """blocks: [{"consensus": str, "members": [edit]}] with edit = {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]};
    who: per block, per member (node_id, reverse) -> {"blocks": every output block {"consensus", "members"}, "orphans": [...] as
    DetachOut.orphans(), "member_map": [...]}"""
    K = _Packed(blocks, [])
    out = detach_unaligned_raw(K.args()[:7], [w for blk in who for w in blk], dll, keep=K)
    try:
        return {"blocks": out.to_dicts(K.L), "orphans": out.orphans(), "member_map": out.member_map()}
    finally:
        out.free()


# ---------------------------------------------------------------- the graph level: host bookkeeping, O(orphans)
def detach_graph(graph, block_ids, dll=None, detach=None):
    """graph: in the shape of simplify.normalize() (changed in place and returned); block_ids: the recently merged (or realigned) blocks.
    Their unaligned nodes leave them; each gets a singleton block whose id is id((node_id, &seq)); its node keeps its id, its path and its
    position, and is forward (detach_unaligned.rs:42-54, 105-111).  detach: stands in for the device call (blocks, who as
    detach_unaligned takes them -> its result)."""
    g = graph
    block_ids = list(block_ids)
    order = [sorted(g["blocks"][b]["alignments"]) for b in block_ids]
    blocks = [{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in nodes]} for b, nodes in zip(block_ids, order)]
    who = [[(n, g["nodes"][n]["strand"] == "-") for n in nodes] for nodes in order]
    res = (detach or (lambda bl, w: detach_unaligned(bl, w, dll)))(blocks, who)
    flat = [(b, n) for b, nodes in zip(block_ids, order) for n in nodes]
    for o in res["orphans"]:
        bid, nid = flat[o["member"]]
        assert nid == o["node_id"]
        if o["status"] != 0:
            raise DetachError(f"node {nid} of block {bid}: " + ("a letter without a complement" if o["status"] == 2 else "a literal '-' in its sequence"))
        del g["blocks"][bid]["alignments"][nid]
        g["blocks"][o["block_id"]] = {"consensus": o["seq"], "alignments": {nid: {"subs": [], "dels": [], "inss": []}}}
        g["nodes"][nid] = dict(g["nodes"][nid], block_id=o["block_id"], strand="+")
    return g


# ---------------------------------------------------------------- solve_promise's tail: the merged blocks, numpy gathers only
SUB = np.dtype([("pos", "<u4"), ("alt", "<u4")])
DEL = np.dtype([("pos", "<u4"), ("len", "<u4")])
INS = np.dtype([("pos", "<u4"), ("len", "<u4"), ("seq_off", "<u8")])
assert (SUB.itemsize, DEL.itemsize, INS.itemsize) == (C.sizeof(sub_t), C.sizeof(del_t), C.sizeof(ins_t))


def _gather(starts, counts, src):
    """src[starts[k] .. starts[k] + counts[k]) for every k, one after the other"""
    counts = counts.astype(np.int64)
    first = np.cumsum(counts) - counts
    return src[np.repeat(starts.astype(np.int64) - first, counts) + np.arange(int(counts.sum()), dtype=np.int64)]


def merged_blocks(anchor, append):
    """The blocks solve_promise returns (reweave.rs:88-93: alignment_insert of every re-aligned member into its anchor block), for all
    promises of a merge, in the layout pga_detach_unaligned takes.
    anchor: {"cons": [bytes] per block, "n_members": per block, "node_ids": per member, "counts": (members, 3) n_subs / n_dels / n_inss,
             "subs" / "dels" / "inss": arrays of SUB / DEL / INS packed in member order, "ins_seq": bytes} -- the anchor blocks;
    append: {"n_members": per block (promise p goes onto block p), "node_ids": per member, "res": per member (n_subs, n_dels, n_inss,
             sub_off, del_off, ins_off) -- the res[] of pga_solve_promises --, "subs" / "dels" / "inss" / "ins_seq": its four arrays}.
    -> a dict like `anchor`: per block the members of both in NodeId (BTreeMap) order, the lists gathered, one ins_seq (the anchor's
    letters followed by the promises': the seq_off of a re-aligned member's insertions moves up by len(anchor["ins_seq"]))."""
    nb = len(anchor["cons"])
    an, pn = np.asarray(anchor["n_members"], np.int64), np.asarray(append["n_members"], np.int64)
    assert len(an) == len(pn) == nb
    a_counts = np.asarray(anchor["counts"], np.int64).reshape(-1, 3)
    res = np.asarray(append["res"], np.int64).reshape(-1, 6)
    ids = np.concatenate([np.asarray(anchor["node_ids"], np.uint64), np.asarray(append["node_ids"], np.uint64)])
    blk = np.concatenate([np.repeat(np.arange(nb), an), np.repeat(np.arange(nb), pn)])
    order = np.lexsort((ids, blk))
    if len(order) > 1 and np.any((ids[order][1:] == ids[order][:-1]) & (blk[order][1:] == blk[order][:-1])):
        raise ValueError("a node id appears twice in one merged block")
    counts = np.concatenate([a_counts, res[:, :3]])[order]
    out = {"cons": list(anchor["cons"]), "n_members": (an + pn).tolist(), "node_ids": ids[order], "counts": counts.astype(np.uint32),
           "ins_seq": bytes(anchor["ins_seq"]) + bytes(append["ins_seq"])}
    for k, (name, dt) in enumerate((("subs", SUB), ("dels", DEL), ("inss", INS))):
        a_src, p_src = np.asarray(anchor[name], dt), np.asarray(append[name], dt).copy()
        if name == "inss":
            p_src["seq_off"] += len(anchor["ins_seq"])
        starts = np.concatenate([np.cumsum(a_counts[:, k]) - a_counts[:, k], res[:, 3 + k] + len(a_src)])[order]
        out[name] = _gather(starts, counts[:, k], np.concatenate([a_src, p_src]))
    return out


class _Arrays:
    """the C view of a merged_blocks() dict; keeps every buffer alive"""

    def __init__(self, a):
        nb = len(a["cons"])
        self.cons = [bytes(c) for c in a["cons"]]
        self.B = (rc_block_t * max(nb, 1))()
        for i, c in enumerate(self.cons):
            self.B[i].consensus = c; self.B[i].cons_len = len(c); self.B[i].n_members = int(a["n_members"][i])
        self.n_blocks, self.n_mem = nb, int(sum(a["n_members"]))
        self.M = np.ascontiguousarray(a["counts"], np.uint32).reshape(-1, 3)
        self.S, self.D, self.I = (np.ascontiguousarray(a[k], dt) for k, dt in (("subs", SUB), ("dels", DEL), ("inss", INS)))
        self.L = C.create_string_buffer(bytes(a["ins_seq"]), max(len(a["ins_seq"]), 1))

    def args(self):
        ptr = lambda x: C.c_void_p(x.ctypes.data) if x.size else None       # (an empty list may be NULL)
        return (self.n_blocks, self.B, ptr(self.M), ptr(self.S), ptr(self.D), ptr(self.I), self.L)


def arrays_args(arrays):
    """a merged_blocks() dict -> (graph_args for detach_unaligned_raw, the object that keeps them alive)"""
    K = _Arrays(arrays)
    return K.args(), K
