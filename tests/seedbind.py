"""ctypes access to the stages in front of chaining and to their expectation (tests only).

 * product (pangraph_amd/libpgalign.so): pga_stage_seed and pga_stage_front_routes (include/pga_align.h): the production build_index_ex,
   index_cal_max_occ / group_mid_occ and seed_all on minimizers given as they are, and the route counters of sketch, index, mid_occ and sort.
 * reference (oracle/_ref/libmm2ref_seed.so: oracle/ref_index_shim.c and oracle/ref_map_shim.c linked in place of index.o and map.o):
   pgref_idx_of_minimizers (mm_idx_add + mm_idx_post), the reference's own mm_idx_cal_max_occ, mm_mapopt_update, mm_seed_mz_flt,
   mm_seed_collect_all, mm_collect_matches, and pgref_collect_seed_hits (collect_seed_hits with skip_seed inside).

A BATCH is what one call of the tap takes: sequences (length, name), groups, per sequence an (n, 2) uint64 array of minimizers in mm_sketch's
layout with the batch-wide sequence index as rid, an optional own mask and the parameter record.  expected(batch) is what the tap must return,
from the reference's own code; every group gets an index of its own with group-relative ids, as one find_matches call would build it.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np
import pytest

from pangraph_amd.mm2ffi import mm_mapopt_t
from stagebind import mm128_t, mm128_v, _libc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SEED_SO = os.path.join(ROOT, "oracle", "_ref", "libmm2ref_seed.so")
_REF_SEED = []

MM_F_NO_DIAG, MM_F_NO_DUAL, MM_F_FOR_ONLY, MM_F_REV_ONLY = 0x001, 0x002, 0x100000, 0x200000
SEED_TANDEM, SEED_SELF = 1 << 42, 1 << 43
ST_DROPPED, ST_USED, ST_FILTERED, ST_TANDEM = 0, 1, 2, 4
ROUTES = ("sk_tiles8_19", "sk_tiles8_10", "sk_tiles", "sk_serial", "sk_retry", "idx_one_sort", "idx_two_sorts", "mo_hist", "mo_sort", "replay_q")
MO_BINS, MO_KEYS = 1024, 2048          # pga_maxocc_hist.h


class pga_seed_params_t(C.Structure):  # include/pga_align.h
    _fields_ = [("flag", C.c_int64)] + [(n, C.c_int32) for n in ("mid_occ", "min_mid_occ", "max_mid_occ", "max_max_occ", "occ_dist", "w", "k")] + \
               [("mid_occ_frac", C.c_float), ("q_occ_frac", C.c_float), ("pad", C.c_int32)]


class mm_seed_t(C.Structure):  # mmpriv.h:40-46
    _fields_ = [("n", C.c_uint32), ("q_pos", C.c_uint32), ("q_span", C.c_uint32, 31), ("flt", C.c_uint32, 1),
                ("seg_id", C.c_uint32, 31), ("is_tandem", C.c_uint32, 1), ("cr", C.POINTER(C.c_uint64))]


# the asm presets' values (options.c:14-64 and the asm branch of mm_set_opt) for everything the stages read; flag: pangraph's pair
DEFAULTS = dict(flag=MM_F_NO_DIAG | MM_F_NO_DUAL, mid_occ=0, min_mid_occ=50, max_mid_occ=500, max_max_occ=4095, occ_dist=500, w=19, k=19,
                mid_occ_frac=2e-4, q_occ_frac=0.01)


@dataclass
class Batch:
    name: str
    lens: list
    names: list                   # bytes
    grp_off: list
    mz: list                      # per sequence: (n, 2) uint64
    params: dict = field(default_factory=dict)
    own: object = None            # None or a list of 0 / 1 per sequence
    pins: dict = field(default_factory=dict)      # what the case was built to hit: checked on the reference by tests/test_seed_cases_cpu.py

    def par(self):
        return {**DEFAULTS, **self.params}

    @property
    def n_seq(self):
        return len(self.lens)

    @property
    def n_grp(self):
        return len(self.grp_off) - 1


def minimizers(k, rid, recs):
    """recs: (hash, position, strand) in ascending position -> (n, 2) uint64 in mm_sketch's layout"""
    a = np.zeros((len(recs), 2), dtype=np.uint64)
    for j, (h, pos, strand) in enumerate(recs):
        a[j, 0] = h << 8 | k
        a[j, 1] = rid << 32 | pos << 1 | strand
    return a


def ref_seed_dll():
    """the library with both shims, built where the reference's sources are present (oracle/Makefile: ref); a skip only if oracle/_ref/ was not
    built and the sources are absent"""
    if not _REF_SEED:
        if not os.path.exists(REF_SEED_SO):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, stdout=subprocess.DEVNULL)
            if not os.path.exists(REF_SEED_SO):
                pytest.skip("oracle/_ref/libmm2ref_seed.so not built and the reference's sources absent")
        d = C.CDLL(REF_SEED_SO)
        d.pgref_idx_of_minimizers.restype = C.c_void_p
        d.pgref_idx_of_minimizers.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_void_p]
        d.mm_idx_destroy.argtypes = [C.c_void_p]
        d.mm_idx_destroy.restype = None
        d.mm_idx_cal_max_occ.restype = C.c_int32
        d.mm_idx_cal_max_occ.argtypes = [C.c_void_p, C.c_float]
        d.mm_mapopt_update.restype = None
        d.mm_mapopt_update.argtypes = [C.POINTER(mm_mapopt_t), C.c_void_p]
        d.mm_seed_mz_flt.restype = None
        d.mm_seed_mz_flt.argtypes = [C.c_void_p, C.POINTER(mm128_v), C.c_int32, C.c_float]
        d.mm_seed_collect_all.restype = C.POINTER(mm_seed_t)
        d.mm_seed_collect_all.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(mm128_v), C.POINTER(C.c_int32)]
        d.mm_collect_matches.restype = C.POINTER(mm_seed_t)
        d.mm_collect_matches.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(mm128_v),
                                         C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.POINTER(C.c_uint64))]
        d.pgref_collect_seed_hits.restype = C.c_int64
        d.pgref_collect_seed_hits.argtypes = [C.POINTER(mm_mapopt_t), C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_int,
                                              C.POINTER(C.c_int), C.c_void_p, C.c_int64]
        _REF_SEED.append(d)
    return _REF_SEED[0]


# ---------------------------------------------------------------- reference
def _ref_opt(p, mid_occ):
    o = mm_mapopt_t()
    o.flag, o.mid_occ, o.mid_occ_frac, o.min_mid_occ, o.max_mid_occ = p["flag"], mid_occ, p["mid_occ_frac"], p["min_mid_occ"], p["max_mid_occ"]
    o.max_max_occ, o.occ_dist, o.q_occ_frac = p["max_max_occ"], p["occ_dist"], p["q_occ_frac"]
    o.bw = o.bw_long = 500
    return o


class RefIndex:
    """the reference's own index of ONE group (group-relative ids), from its minimizers"""

    def __init__(self, B, g):
        d = ref_seed_dll()
        p = B.par()
        self.b, self.e = B.grp_off[g], B.grp_off[g + 1]
        parts = [B.mz[i] for i in range(self.b, self.e)]
        a = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.uint64)
        a = np.ascontiguousarray(a).copy()
        a[:, 1] -= np.uint64(self.b << 32)
        self.n_mz = len(a)
        n = self.e - self.b
        names = (C.c_char_p * max(n, 1))(*B.names[self.b:self.e])
        lens = np.ascontiguousarray(np.array(B.lens[self.b:self.e], dtype=np.uint32))
        self.mi = d.pgref_idx_of_minimizers(p["w"], p["k"], len(a), a.ctypes.data, n, names, lens.ctypes.data)
        self.d = d

    def close(self):
        self.d.mm_idx_destroy(self.mi)


def clamp_mid_occ(raw, p):  # options.c:66-80
    m = raw
    if m < p["min_mid_occ"]:
        m = p["min_mid_occ"]
    if p["max_mid_occ"] > p["min_mid_occ"] and m > p["max_mid_occ"]:
        m = p["max_mid_occ"]
    return m


def ref_mid_occ(B, g, X=None):
    """(raw, mid_occ) of group g: mm_idx_cal_max_occ and mm_mapopt_update.  A group without a minimizer: the reference would select from an
    empty array (index.c:195-204 on n = 0); the project defines raw = 1 there, and so does this function, with the clamps of options.c."""
    p = B.par()
    own = X is None
    X = X or RefIndex(B, g)
    try:
        if X.n_mz == 0:
            raw = 1
            mid = p["mid_occ"] if p["mid_occ"] > 0 else clamp_mid_occ(raw, p)
        else:
            raw = X.d.mm_idx_cal_max_occ(X.mi, p["mid_occ_frac"])
            o = _ref_opt(p, p["mid_occ"])
            X.d.mm_mapopt_update(C.byref(o), X.mi)
            mid = o.mid_occ
    finally:
        if own:
            X.close()
    return raw, mid


def expected(B):
    """what pga_stage_seed must return for batch B in mode 0, and what a test needs to pin: dict with mid_occ, raw (per group), state (per
    sequence), rep_len, anchors (per sequence, (n, 2) uint64 in the reference's final order), n_kept (per sequence)"""
    if "_expected" in B.__dict__:
        return B.__dict__["_expected"]
    d = ref_seed_dll()
    p = B.par()
    E = dict(mid_occ=[], raw=[], state=[None] * B.n_seq, rep_len=[0] * B.n_seq, anchors=[None] * B.n_seq, n_kept=[0] * B.n_seq)
    for g in range(B.n_grp):
        X = RefIndex(B, g)
        raw, mid = ref_mid_occ(B, g, X)
        E["raw"].append(raw)
        E["mid_occ"].append(mid)
        o = _ref_opt(p, mid)
        for i in range(X.b, X.e):
            n = len(B.mz[i])
            st = np.zeros(n, dtype=np.uint8)
            E["state"][i], E["anchors"][i] = st, np.zeros((0, 2), dtype=np.uint64)
            if (B.own is not None and not B.own[i]) or n == 0:
                continue
            a = np.ascontiguousarray(B.mz[i]).copy()
            a[:, 1] &= np.uint64(0xffffffff)          # mm_map_frag sketches a query with rid 0 (map.c:66): the upper half is the segment id
            mv = mm128_v(n, n, C.cast(a.ctypes.data, C.POINTER(mm128_t)))
            d.mm_seed_mz_flt(None, C.byref(mv), mid, p["q_occ_frac"])
            nk = mv.n
            E["n_kept"][i] = nk
            kept = np.searchsorted(B.mz[i][:, 1] & np.uint64(0xffffffff), a[:nk, 1])     # positions ascend: y identifies the minimizer
            assert np.array_equal(B.mz[i][kept, 0], a[:nk, 0])
            if nk == 0:
                continue
            mv.m = nk
            n0 = C.c_int32(0)
            m = d.mm_seed_collect_all(None, X.mi, C.byref(mv), C.byref(n0))
            assert n0.value == nk                                                        # every query minimizer is indexed
            tandem = np.array([m[j].is_tandem for j in range(nk)], dtype=np.uint8)
            _libc.free(m)
            n_m, n_a, rl, nmp, mp = C.c_int(0), C.c_int64(0), C.c_int(0), C.c_int(0), C.POINTER(C.c_uint64)()
            m = d.mm_collect_matches(None, C.byref(n_m), B.lens[i], mid, p["max_max_occ"], p["occ_dist"], X.mi, C.byref(mv), C.byref(n_a), C.byref(rl),
                                     C.byref(nmp), C.byref(mp))
            used = set(m[j].q_pos for j in range(n_m.value))
            _libc.free(m)
            _libc.free(mp)
            for j in range(nk):
                st[kept[j]] = (ST_USED if int(a[j, 1]) in used else ST_FILTERED) | (ST_TANDEM if tandem[j] else 0)
            out = np.zeros((max(n_a.value, 1), 2), dtype=np.uint64)
            rl2 = C.c_int(0)
            na = d.pgref_collect_seed_hits(C.byref(o), mid, X.mi, B.names[i], nk, a.ctypes.data, B.lens[i], C.byref(rl2), out.ctypes.data, len(out))
            assert na <= n_a.value and rl2.value == rl.value
            E["rep_len"][i] = rl.value
            E["anchors"][i] = out[:na].copy()
        X.close()
    B.__dict__["_expected"] = E
    return E


def stable_order(a):
    """a query's anchors as a stable sort by x of the generation order leaves them: equal x come from different seeds of the query, in query
    order -- ascending query position on the forward strand, descending on the reverse strand (map.c:190)"""
    if len(a) == 0:
        return a
    x, qp = a[:, 0], (a[:, 1] & np.uint64(0xffffffff)).astype(np.int64)
    sec = np.where(x >> np.uint64(63) != 0, -qp, qp)
    return a[np.lexsort((sec, x))]


def has_tie(a):
    return bool(len(a) > 1 and (np.sort(a[:, 0])[1:] == np.sort(a[:, 0])[:-1]).any())


def expected_routes(B, E):
    """the route counters one mode-0 call of the tap must leave, from the reference's answers and the kernels' stated thresholds"""
    p = B.par()
    n_mz = sum(len(m) for m in B.mz)
    gbits = (B.n_grp - 1).bit_length()
    two = min(64, 2 * p["k"]) + gbits > 64
    derive = p["mid_occ"] <= 0 and n_mz > 0 and p["mid_occ_frac"] > 0
    sort = derive and any(r - 1 >= MO_BINS - 1 for r in E["raw"])
    return dict(idx_one_sort=int(n_mz > 0 and not two), idx_two_sorts=int(n_mz > 0 and two), mo_hist=int(derive and not sort), mo_sort=int(sort),
                replay_q=sum(has_tie(a) for a in E["anchors"]))


# ---------------------------------------------------------------- product
def _err(dll):
    dll.pga_last_error.restype = C.c_char_p
    return dll.pga_last_error().decode()


def product_seed(dll, B, mode):
    p = B.par()
    n = B.n_seq
    P = pga_seed_params_t()
    for f in ("flag", "mid_occ", "min_mid_occ", "max_mid_occ", "max_max_occ", "occ_dist", "w", "k", "mid_occ_frac", "q_occ_frac"):
        setattr(P, f, p[f])
    lens = np.ascontiguousarray(np.array(B.lens, dtype=np.uint32))
    names = (C.c_char_p * max(n, 1))(*B.names)
    grp = np.ascontiguousarray(np.array(B.grp_off, dtype=np.int64))
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in B.mz])
    flat = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.uint64).reshape(-1, 2) for m in B.mz] + [np.zeros((0, 2), dtype=np.uint64)]))
    own = None if B.own is None else np.ascontiguousarray(np.array(B.own, dtype=np.uint8))
    n_mz = int(off[n])
    mid = np.zeros(max(B.n_grp, 1), dtype=np.int32)
    state = np.full(max(n_mz, 1), 255, dtype=np.uint8)
    rep, tie, aoff = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint32), np.zeros(n + 1, dtype=np.uint64)
    axy = C.POINTER(C.c_uint64)()
    dll.pga_stage_seed.restype = C.c_int
    dll.pga_stage_seed.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_char_p), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(pga_seed_params_t), C.c_int] + [C.c_void_p] * 4 + [C.POINTER(C.POINTER(C.c_uint64)), C.c_void_p]
    rc = dll.pga_stage_seed(n, lens.ctypes.data, names, B.n_grp, grp.ctypes.data, off.ctypes.data, flat.ctypes.data, None if own is None else own.ctypes.data,
                            C.byref(P), mode, mid.ctypes.data, state.ctypes.data, rep.ctypes.data, aoff.ctypes.data, C.byref(axy), tie.ctypes.data)
    if rc != 0:
        raise RuntimeError(_err(dll))
    n_a = int(aoff[n])
    a = np.ctypeslib.as_array(axy, shape=(max(n_a, 1) * 2,))[:n_a * 2].reshape(-1, 2).copy()
    dll.pga_free.argtypes = [C.c_void_p]
    dll.pga_free(axy)
    return dict(mid_occ=mid[:B.n_grp].tolist(), state=[state[int(off[i]):int(off[i + 1])] for i in range(n)], rep_len=rep[:n].tolist(),
                anchors=[a[int(aoff[i]):int(aoff[i + 1])] for i in range(n)], q_tie=tie[:n].tolist())


def product_front_routes(dll):
    """the route counters since the last call (zeroed by the call), by name"""
    out = (C.c_int64 * len(ROUTES))()
    dll.pga_stage_front_routes.restype = None
    dll.pga_stage_front_routes.argtypes = [C.c_void_p]
    dll.pga_stage_front_routes(out)
    return dict(zip(ROUTES, list(out)))
