"""Python host mirror of the merge-promise entry (the whole step): `pga_solve_promises` (include/pga_align.h) replaces
MergePromise::solve_promise (packages/pangraph/src/pangraph/reweave.rs:40-94) for all promises of a merge at once -- consensus sequences, edit
lists, CIGARs and orientations in, every member's edits against its anchor consensus out.  ctypes only; the HIP library does the work."""
import ctypes as C

from . import batch
from .mapvar import del_t, ins_t, params, params_t, res_t, sub_t  # noqa: F401
from .reconsensus import rc_member_t

CIGAR_OPS = "MIDNSHP=XB"


class promise_t(C.Structure):
    _fields_ = [("anchor", C.c_char_p), ("anchor_len", C.c_uint32), ("append", C.c_char_p), ("append_len", C.c_uint32), ("reverse", C.c_int32),
                ("cigar", C.POINTER(C.c_uint32)), ("n_cigar", C.c_uint32), ("n_members", C.c_uint32)]


def pack_cigar(ops):
    """[(len, op letter)] -> minimap2's words, len << 4 | op"""
    return [(ln << 4) | CIGAR_OPS.index(op) for ln, op in ops]


class _Packed:
    """the C arrays of a list of promises; keeps every buffer alive"""

    def __init__(self, promises):
        n = len(promises)
        self.n = n
        cache = {}
        self.P = (promise_t * max(n, 1))()
        self.n_mem = sum(len(q[4]) for q in promises)
        self.M = (rc_member_t * max(self.n_mem, 1))()
        self.keep = []
        subs, dels, inss, letters = [], [], [], bytearray()
        m = 0
        for i, (anchor, append, reverse, cigar_ops, members) in enumerate(promises):
            ab = cache.setdefault(("a", anchor), anchor.encode())     # promises onto the same consensus share one buffer, as the caller's would
            pb = cache.setdefault(("p", append), append.encode())
            words = pack_cigar(cigar_ops)
            cg = (C.c_uint32 * max(len(words), 1))(*words)
            self.keep.append(cg)
            self.P[i].anchor = ab; self.P[i].anchor_len = len(ab); self.P[i].append = pb; self.P[i].append_len = len(pb)
            self.P[i].reverse = 1 if reverse else 0
            self.P[i].cigar = C.cast(cg, C.POINTER(C.c_uint32)); self.P[i].n_cigar = len(words); self.P[i].n_members = len(members)
            for e in members:
                self.M[m].n_subs = len(e["subs"]); self.M[m].n_dels = len(e["dels"]); self.M[m].n_inss = len(e["inss"])
                subs += [(pos, ord(a)) for pos, a in e["subs"]]
                dels += list(e["dels"])
                for pos, seq in e["inss"]:
                    inss.append((pos, len(seq), len(letters)))
                    letters += seq.encode()
                m += 1
        self.keep.append(cache)
        self.S = (sub_t * max(len(subs), 1))(*[sub_t(*x) for x in subs])
        self.D = (del_t * max(len(dels), 1))(*[del_t(*x) for x in dels])
        self.I = (ins_t * max(len(inss), 1))(*[ins_t(*x) for x in inss])
        self.L = C.create_string_buffer(bytes(letters), max(len(letters), 1))
        self.handed_over = sum(len(v) for v in cache.values()) + 8 * len(subs) + 8 * len(dels) + 16 * len(inss) + len(letters)

    def args(self):
        return (self.n, self.P, self.M, self.S, self.D, self.I, self.L)


def solve_promises_raw(promises, p=None, dll=None):
    """-> (res_t array, subs, dels, inss, ins_seq pointers, free()) without unpacking; the caller calls free() when done"""
    p = p or params()
    dll = dll or batch.lib()
    K = _Packed(promises)
    R = (res_t * max(K.n_mem, 1))()
    subs = C.POINTER(sub_t)(); dels = C.POINTER(del_t)(); inss = C.POINTER(ins_t)(); iseq = C.POINTER(C.c_char)()
    dll.pga_solve_promises.restype = C.c_int
    dll.pga_solve_promises.argtypes = [C.c_int64] + [C.c_void_p] * 8 + [C.POINTER(C.POINTER(sub_t)), C.POINTER(C.POINTER(del_t)), C.POINTER(C.POINTER(ins_t)), C.POINTER(C.POINTER(C.c_char))]
    dll.pga_last_error.restype = C.c_char_p
    dll.pga_free.argtypes = [C.c_void_p]
    if dll.pga_solve_promises(*K.args(), C.byref(p), R, C.byref(subs), C.byref(dels), C.byref(inss), C.byref(iseq)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())

    def free():
        for ptr in (subs, dels, inss, iseq):
            if ptr:
                dll.pga_free(C.cast(ptr, C.c_void_p))
    return K, R, subs, dels, inss, iseq, free


def solve_promises(promises, p=None, dll=None):
    """promises: [(anchor consensus, append consensus, reverse, [(len, op letter)], [edit, ...])] with
    edit = {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]} against the append consensus, members in the reference's
    BTreeMap order.  -> per promise a list with one dict per member, as pangraph_amd.mapvar.map_variations returns them (status, score,
    attempts, hit_boundary, subs, dels, inss -- the edits against the ANCHOR consensus)"""
    K, R, subs, dels, inss, iseq, free = solve_promises_raw(promises, p, dll)
    out = []
    try:
        base = C.addressof(iseq.contents)
        m = 0
        for q in promises:
            rows = []
            for _ in q[4]:
                r = R[m]
                rows.append(dict(status=r.status, score=r.score, attempts=r.attempts, hit_boundary=r.hit_boundary,
                                 subs=[(subs[r.sub_off + k].pos, chr(subs[r.sub_off + k].alt)) for k in range(r.n_subs)],
                                 dels=[(dels[r.del_off + k].pos, dels[r.del_off + k].len) for k in range(r.n_dels)],
                                 inss=[(inss[r.ins_off + k].pos, C.string_at(base + inss[r.ins_off + k].seq_off, inss[r.ins_off + k].len).decode()) for k in range(r.n_inss)]))
                m += 1
            out.append(rows)
    finally:
        free()
    return out


def stage_jobs(promises, dll=None):
    """the stage tap pga_stage_promise_jobs: per promise a list with one (status, mean_shift, band_width, oriented sequence) per member --
    what solve_promise has worked out when it calls map_variations (band before extra_band_width; "" where the status is not 0)"""
    dll = dll or batch.lib()
    K = _Packed(promises)
    n = max(K.n_mem, 1)
    status = (C.c_int32 * n)(); ms = (C.c_int32 * n)(); bw = (C.c_uint32 * n)(); off = (C.c_uint64 * (n + 1))()
    seqs = C.POINTER(C.c_char)()
    dll.pga_stage_promise_jobs.restype = C.c_int
    dll.pga_stage_promise_jobs.argtypes = [C.c_int64] + [C.c_void_p] * 10 + [C.POINTER(C.POINTER(C.c_char))]
    dll.pga_last_error.restype = C.c_char_p
    dll.pga_free.argtypes = [C.c_void_p]
    if dll.pga_stage_promise_jobs(*K.args(), status, ms, bw, off, C.byref(seqs)) != 0:
        raise batch.PgaError(dll.pga_last_error().decode())
    out = []
    try:
        base = C.addressof(seqs.contents)
        m = 0
        for q in promises:
            rows = []
            for _ in q[4]:
                rows.append((status[m], ms[m], bw[m], C.string_at(base + off[m], off[m + 1] - off[m]).decode()))
                m += 1
            out.append(rows)
    finally:
        if seqs:
            dll.pga_free(C.cast(seqs, C.c_void_p))
    return out
