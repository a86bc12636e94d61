"""Python host mirror of the slicing entry: `pga_slice_blocks` (include/pga_align.h) replaces block_slice (packages/pangraph/src/pangraph/
slice.rs:12-202) for every interval of every block a merge cuts (reweave.rs:342-402, 427-438) -- blocks with their members' edit lists, old
nodes and interval tables in, per (block, interval) the kept members with sliced edits, coordinates, new position and strand, and the
dropped members out.  ctypes only; the HIP library does the work."""
import ctypes as C

from . import batch
from .mapvar import del_t, ins_t, sub_t
from .reconsensus import rc_member_t


class slice_block_t(C.Structure):
    _fields_ = [("consensus", C.c_char_p), ("cons_len", C.c_uint32), ("n_members", C.c_uint32), ("n_intervals", C.c_uint32)]


class slice_interval_t(C.Structure):
    _fields_ = [("start", C.c_uint32), ("end", C.c_uint32), ("flip", C.c_int32)]


class slice_node_t(C.Structure):
    _fields_ = [("pos_start", C.c_uint64), ("pos_end", C.c_uint64), ("path_len", C.c_uint64), ("reverse", C.c_int32), ("circular", C.c_int32)]


class slice_member_t(C.Structure):
    _fields_ = [("member", C.c_uint32), ("reverse", C.c_int32), ("node_start", C.c_uint32), ("node_end", C.c_uint32),
                ("pos_start", C.c_uint64), ("pos_end", C.c_uint64), ("counts", rc_member_t),
                ("sub_off", C.c_uint64), ("del_off", C.c_uint64), ("ins_off", C.c_uint64)]


class slice_res_t(C.Structure):
    _fields_ = [("member_off", C.c_uint64), ("n_kept", C.c_uint32), ("n_dropped", C.c_uint32)]


class slice_out_t(C.Structure):
    _fields_ = [("slices", C.POINTER(slice_res_t)), ("members", C.POINTER(slice_member_t)), ("counts", C.POINTER(rc_member_t)), ("dropped", C.POINTER(C.c_uint32)),
                ("subs", C.POINTER(sub_t)), ("dels", C.POINTER(del_t)), ("inss", C.POINTER(ins_t))]


class _Packed:
    """the C arrays of a list of blocks; keeps every buffer alive"""

    def __init__(self, blocks):
        nb = len(blocks)
        self.n = nb
        self.cons = [b["consensus"].encode() for b in blocks]
        self.n_mem = sum(len(b["members"]) for b in blocks)
        self.n_int = sum(len(b["intervals"]) for b in blocks)
        self.B = (slice_block_t * max(nb, 1))()
        self.V = (slice_interval_t * max(self.n_int, 1))()
        self.M = (rc_member_t * max(self.n_mem, 1))()
        self.N = (slice_node_t * max(self.n_mem, 1))()
        subs, dels, inss, letters = [], [], [], bytearray()
        m = v = 0
        for i, b in enumerate(blocks):
            assert len(b["nodes"]) == len(b["members"])
            self.B[i].consensus = self.cons[i]; self.B[i].cons_len = len(self.cons[i]); self.B[i].n_members = len(b["members"]); self.B[i].n_intervals = len(b["intervals"])
            for start, end, flip in b["intervals"]:
                self.V[v].start = start; self.V[v].end = end; self.V[v].flip = 1 if flip else 0
                v += 1
            for e, node in zip(b["members"], b["nodes"]):
                self.M[m].n_subs = len(e["subs"]); self.M[m].n_dels = len(e["dels"]); self.M[m].n_inss = len(e["inss"])
                self.N[m].pos_start, self.N[m].pos_end, self.N[m].path_len = node[0], node[1], node[2]
                self.N[m].reverse = 1 if node[3] else 0; self.N[m].circular = 1 if node[4] else 0
                subs += [(pos, ord(a)) for pos, a in e["subs"]]
                dels += list(e["dels"])
                for pos, seq in e["inss"]:
                    inss.append((pos, len(seq), len(letters)))
                    letters += seq.encode()
                m += 1
        self.S = (sub_t * max(len(subs), 1))(*[sub_t(*x) for x in subs])
        self.D = (del_t * max(len(dels), 1))(*[del_t(*x) for x in dels])
        self.I = (ins_t * max(len(inss), 1))(*[ins_t(*x) for x in inss])
        self.L = C.create_string_buffer(bytes(letters), max(len(letters), 1))     # the caller's ins_seq: pga_slice_blocks never sees it
        self.n_edits = len(subs) + len(dels) + len(inss)

    def args(self):
        return (self.n, self.B, self.V, self.M, self.N, self.S, self.D, self.I)


def _bind(dll):
    dll.pga_slice_blocks.restype = C.c_int
    dll.pga_slice_blocks.argtypes = [C.c_int64] + [C.c_void_p] * 8
    dll.pga_slice_free.restype = None
    dll.pga_slice_free.argtypes = [C.c_void_p]
    dll.pga_last_error.restype = C.c_char_p


def slice_blocks_raw(blocks, dll=None):
    """-> (packed input, slice_out_t, free()) without unpacking; the caller calls free() when done"""
    dll = dll or batch.lib()
    _bind(dll)
    K = _Packed(blocks)
    out = slice_out_t()
    if dll.pga_slice_blocks(*K.args(), C.byref(out)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    return K, out, lambda: dll.pga_slice_free(C.byref(out))


def slice_blocks(blocks, dll=None):
    """blocks: [{"consensus": str, "members": [edit, ...], "nodes": [(pos_start, pos_end, path_len, reverse, circular), ...],
    "intervals": [(start, end, flip), ...]}] with edit = {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]}, members in the
    reference's BTreeMap order, nodes parallel to them (the OLD node of every member), flip = aligned and not is_anchor and the orientation is
    reverse.  -> per block a list with one dict per interval: member_off, kept = [dict(member, reverse, node, pos, subs, dels, inss, sub_off,
    del_off, ins_off)] in member order, dropped = [member index, ...].  The consensus of a slice is consensus[start:end]."""
    K, out, free = slice_blocks_raw(blocks, dll)
    res = []
    try:
        letters = K.L.raw
        s = drop0 = 0
        for b in blocks:
            rows = []
            for _ in b["intervals"]:
                r = out.slices[s]
                kept = []
                for k in range(r.member_off, r.member_off + r.n_kept):
                    v = out.members[k]
                    c = out.counts[k]
                    assert (c.n_subs, c.n_dels, c.n_inss) == (v.counts.n_subs, v.counts.n_dels, v.counts.n_inss)
                    kept.append(dict(member=v.member, reverse=bool(v.reverse), node=(v.node_start, v.node_end), pos=(v.pos_start, v.pos_end),
                                     subs=[(out.subs[v.sub_off + t].pos, chr(out.subs[v.sub_off + t].alt)) for t in range(c.n_subs)],
                                     dels=[(out.dels[v.del_off + t].pos, out.dels[v.del_off + t].len) for t in range(c.n_dels)],
                                     inss=[(x.pos, letters[x.seq_off:x.seq_off + x.len].decode()) for x in (out.inss[v.ins_off + t] for t in range(c.n_inss))],
                                     sub_off=v.sub_off, del_off=v.del_off, ins_off=v.ins_off))
                rows.append(dict(member_off=r.member_off, kept=kept, dropped=[out.dropped[drop0 + t] for t in range(r.n_dropped)]))
                drop0 += r.n_dropped
                s += 1
            res.append(rows)
    finally:
        free()
    return res
