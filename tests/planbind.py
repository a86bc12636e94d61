"""ctypes access to the region planner and to its expectation (tests only).

 * product (pangraph_amd/libpgalign.so): pga_stage_plan (include/pga_align.h), the production plan_regions of pga_plan.hip on explicit inputs.
 * reference (oracle/_ref/libmm2ref_plan.so: oracle/ref_align_shim.c compiled with -DPGREF_PLAN_TRACE): pgref_chain_extent (mm_gen_regs), pgref_trim_and_filter (mm_fix_bad_ends and
   both seed filters) and pgref_align1_trace (mm_align1 itself with the DP replaced by logging stand-ins).

A GROUP is what one call of the tap takes: sequences (numpy uint8 base codes 0..4), the first sequence of the group inside them, queries with their
anchor arrays ((n, 2) uint64: x = strand<<63 | target<<32 | target position, y = flags | span<<32 | position on the aligned strand), regions
(query, as, cnt) and the planner's parameters.  expected(group) is what the tap must return, from the reference's own code: extent from
mm_gen_regs; as1 / cnt1, the windows, the segment list, T_re / T_qe and the flags from the log of mm_align1's DP calls; probes and runs, the
project's own shortcut, as plain numpy over that segment list.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np
import pytest

from pangraph_amd.mm2ffi import mm_mapopt_t, mm_idx_t
from postbind import revcomp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PLAN_SO = os.path.join(ROOT, "oracle", "_ref", "libmm2ref_plan.so")
_REF_PLAN = []


def ref_plan_dll():
    """the shim library with the logging stand-ins, built where the reference's sources are present (oracle/Makefile: ref); a skip only if
    oracle/_ref/ was not built"""
    if not _REF_PLAN:
        if not os.path.exists(REF_PLAN_SO):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, stdout=subprocess.DEVNULL)
            if not os.path.exists(REF_PLAN_SO):
                pytest.skip("oracle/_ref/libmm2ref_plan.so not built and the reference's sources absent")
        _REF_PLAN.append(C.CDLL(REF_PLAN_SO))
    return _REF_PLAN[0]

A_LONG_JOIN, A_IGNORE, A_TANDEM, A_SELF = 1 << 40, 1 << 41, 1 << 42, 1 << 43
MM_F_NO_END_FLT = 0x10000000
KSW_EZ_RIGHT, KSW_EZ_EXTZ_ONLY = 0x02, 0x40
G_MAX_KERNEL = 4096


class PlanParams(C.Structure):  # pga_plan.h: PlanParams
    _fields_ = [(n, C.c_int32) for n in ("k", "bw", "bw_long", "max_gap", "min_cnt", "min_chain_score", "min_ksw_len", "a", "q", "e", "no_end_flt",
                                         "probe_m_max", "g_max", "pad")] + [("max_sw_mat", C.c_int64)]


OUT_FIELDS = ("status", "rid", "rev", "r_rs", "r_re", "r_qs", "r_qe", "r_mlen", "r_blen", "as1", "cnt1", "rs", "qs", "rs0", "qs0", "re0", "qe0",
              "T_re", "T_qe", "n_items", "n_long_gaps")
EXTENT_FIELDS = OUT_FIELDS[1:9]
ITEM_FIELDS = ("kind", "i", "rs", "qs", "re", "qe", "bw1", "m", "i_prev")


class PlanOut(C.Structure):  # pga_plan.h: PlanOut
    _fields_ = [(n, C.c_uint32 if n == "n_items" else C.c_int32) for n in OUT_FIELDS]


class PlanItem(C.Structure):  # pga_plan.h: PlanItem
    _fields_ = [(n, C.c_int32) for n in ITEM_FIELDS] + [("pad", C.c_int32 * 3)]


class PlanIn(C.Structure):  # pga_plan.h: PlanIn (the tap fills it; mirrored for the layout test)
    _fields_ = [("a_off", C.c_uint64), ("item_off", C.c_uint64), ("item_cap", C.c_uint32), ("n_a", C.c_int32), ("as_", C.c_int32), ("cnt", C.c_int32),
                ("qlen", C.c_int32), ("qid", C.c_int32), ("base", C.c_int32), ("pad", C.c_int32)]


DEFAULTS = dict(k=15, bw=500, bw_long=20000, max_gap=5000, min_cnt=3, min_chain_score=40, min_ksw_len=200, a=2, b=4, q=4, e=2, q2=24, e2=1,
                no_end_flt=0, probe_m_max=2, g_max=G_MAX_KERNEL, max_sw_mat=100_000_000)


@dataclass
class Group:
    name: str
    seqs: list                    # numpy uint8 arrays, the whole store in order
    base: int                     # sequences [base, len(seqs)) are the group: target id t is seqs[base + t]
    queries: list                 # (index into seqs, anchors (n, 2) uint64)
    regions: list                 # (query index, as, cnt)
    params: dict = field(default_factory=dict)
    pins: dict = field(default_factory=dict)      # what the case was built to hit: checked on the reference by tests/test_plan_cases_cpu.py

    def par(self):
        return {**DEFAULTS, **self.params}


def anchor(rev, rid, tpos, qpos, span=15, flags=0):
    return (rev << 63 | rid << 32 | tpos, flags | span << 32 | qpos)


def anchors_array(lst):
    return np.ascontiguousarray(np.array(lst, dtype=np.uint64).reshape(-1, 2))


def tpos(a):
    return (a[:, 0] & 0xffffffff).astype(np.int64)


def qpos(a):
    return (a[:, 1] & 0xffffffff).astype(np.int64)


def flags(a):
    return a[:, 1] & np.uint64(0xf << 40)


def bw_long_of(p):
    return max(int(p["bw_long"] * 1.5 + 1.), int(p["bw"] * 1.5 + 1.))      # align.c:590-592


def plan_params(p):
    P = PlanParams()
    for n in ("k", "bw", "max_gap", "min_cnt", "min_chain_score", "min_ksw_len", "a", "q", "e", "no_end_flt", "probe_m_max", "g_max", "max_sw_mat"):
        setattr(P, n, p[n])
    P.bw_long = bw_long_of(p)
    return P


# ---------------------------------------------------------------- reference
def _opt(p):
    o = mm_mapopt_t()
    C.memset(C.byref(o), 0, C.sizeof(o))
    for n in ("bw", "bw_long", "max_gap", "min_cnt", "min_chain_score", "min_ksw_len", "a", "b", "q", "e", "q2", "e2"):
        setattr(o, n, p[n])
    o.sc_ambi, o.end_bonus, o.zdrop, o.zdrop_inv = 1, -1, 1 << 29, 1 << 29      # (the bookkeeping lists of the stand-ins must never look z-dropped)
    o.flag = MM_F_NO_END_FLT if p["no_end_flt"] else 0
    o.max_sw_mat = 0                                                             # every segment reaches the stand-in
    return o


_IDX = {}


def ref_index(G):
    """mm_idx_str over the group's sequences (kept for the process: a group is read-only)"""
    if G.name not in _IDX:
        d = ref_plan_dll()
        d.mm_idx_str.restype = C.POINTER(mm_idx_t)
        d.mm_idx_str.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p]
        grp = G.seqs[G.base:]
        strs = [bytes(np.frombuffer(b"ACGTN", np.uint8)[np.minimum(s, 4)]) for s in grp]
        sa = (C.c_char_p * len(grp))(*strs)
        _IDX[G.name] = d.mm_idx_str(10, G.par()["k"], 0, 10, len(grp), C.cast(sa, C.c_void_p), None)
    return _IDX[G.name]


def ref_chain_extent(qlen, a, as_, cnt):
    """mm_gen_regs of one chain -> dict over EXTENT_FIELDS"""
    f = ref_plan_dll().pgref_chain_extent
    f.restype, f.argtypes = None, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    out = np.zeros(8, np.int32)
    f(qlen, a.ctypes.data, as_, cnt, out.ctypes.data)
    r = dict(zip(("rid", "rev", "r_rs", "r_re", "r_qs", "r_qe", "r_mlen", "r_blen"), (int(v) for v in out)))
    return r


def ref_trim_and_filter(qlen, a, as_, cnt, p):
    """mm_fix_bad_ends and both seed filters on a (flagged in place) -> (as1, cnt1)"""
    f = ref_plan_dll().pgref_trim_and_filter
    f.restype, f.argtypes = None, [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    out = np.zeros(2, np.int32)
    f(qlen, a.ctypes.data, as_, cnt, p["bw"], p["min_chain_score"], p["max_gap"], p["no_end_flt"], out.ctypes.data)
    return int(out[0]), int(out[1])


def ref_align1_trace(G, q_index, a, as_, cnt):
    """the DP calls mm_align1 makes for the chain a[as .. as + cnt) (a is flagged in place) -> (n, 8) int32:
    strand, query offset, qlen, tlen, w, zdrop, end_bonus, flag"""
    f = ref_plan_dll().pgref_align1_trace
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64]
    q = np.ascontiguousarray(G.seqs[q_index], np.uint8)
    log = np.zeros((cnt + 3, 8), np.int32)
    o = _opt(G.par())
    n = f(C.addressof(o), ref_index(G), len(q), q.ctypes.data, len(a), a.ctypes.data, as_, cnt, log.ctypes.data, len(log))
    assert 0 <= n <= len(log), f"{G.name}: mm_align1 made {n} DP calls for {cnt} anchors"
    return log[:n]


# ---------------------------------------------------------------- the project's own shortcut: plain numpy
def probe(t_win, q_win, m_max):
    """the identity probe of two equally long windows on the aligned strand: mismatches, or -1 for a code above 3 or more than m_max of them"""
    t_win, q_win = np.asarray(t_win), np.asarray(q_win)
    if (t_win > 3).any() or (q_win > 3).any():
        return -1
    m = int((t_win != q_win).sum())
    return m if m <= m_max else -1


def n_long_gaps(a, as1, cnt1, min_gap=10):
    c = a[as1:as1 + cnt1]
    g = np.diff(qpos(c)) - np.diff(tpos(c))
    return int((np.abs(g) > min_gap).sum())


def collapse(segs, target, q_aligned, p):
    """segs: dicts(i, i_prev, rs, qs, re, qe, bw1) in chain order -> items as (m, 9) int32 in ITEM_FIELDS order"""
    items, run = [], None
    for s in segs:
        ql, tl = s["qe"] - s["qs"], s["re"] - s["rs"]
        eligible = ql == tl and s["bw1"] >= ql
        probed = eligible and p["probe_m_max"] >= 0 and ql > 0 and (p["max_sw_mat"] <= 0 or ql * tl <= p["max_sw_mat"])
        m = probe(target[s["rs"]:s["re"]], q_aligned[s["qs"]:s["qe"]], p["probe_m_max"]) if probed else -1
        if m >= 0:
            if run is None:
                run = dict(kind=0, rs=s["rs"], qs=s["qs"], i_prev=s["i_prev"], bw1=0, m=0)
            run.update(i=s["i"], re=s["re"], qe=s["qe"], bw1=run["bw1"] + 1, m=run["m"] + m)
            continue
        if run is not None:
            items.append(run)
            run = None
        items.append(dict(s, kind=2 if eligible else 1, m=0))
    if run is not None:
        items.append(run)
    return np.array([[it[f] for f in ITEM_FIELDS] for it in items], np.int32).reshape(-1, 9)


# ---------------------------------------------------------------- expectation
def parse_trace(log, a, as_, cnt, half_k, rev):
    """the log of one region -> dict(as1, cnt1, rs, qs, rs0, qs0, re0, qe0, T_re, T_qe, segs); None for what the log cannot say (as1 of a chain whose
    mm_align1 made no DP call at all)"""
    assert (log[:, 0] == rev).all(), "a DP call on the other strand"
    ext = (log[:, 7] & KSW_EZ_EXTZ_ONLY) != 0
    left = log[0] if len(log) and ext[0] and log[0, 7] & KSW_EZ_RIGHT else None
    right = log[-1] if len(log) and ext[-1] and not log[-1, 7] & KSW_EZ_RIGHT else None
    mid = log[(left is not None):len(log) - (right is not None)]
    assert not ((mid[:, 7] & KSW_EZ_EXTZ_ONLY) != 0).any(), "an extension between the gap-fill calls"
    if len(mid):
        qs = int(mid[0, 1])
    elif left is not None:
        qs = int(left[1] + left[2])
    elif right is not None:
        qs = int(right[1])
    else:
        return None
    qp, tp = qpos(a) - half_k, tpos(a) - half_k
    chain = np.arange(as_, as_ + cnt)
    hit = chain[qp[chain] == qs]
    assert len(hit) == 1, "the first DP call starts at no anchor of the chain"
    as1 = int(hit[0])
    rs = int(tp[as1])
    segs, q, t, i_prev = [], qs, rs, 0
    for r in mid:
        assert int(r[1]) == q, "gap-fill calls do not follow each other on the query"
        qe, te = q + int(r[2]), t + int(r[3])
        hit = chain[(qp[chain] == qe) & (tp[chain] == te)]
        assert len(hit) == 1, "a gap-fill call ends at no anchor of the chain"
        i = int(hit[0]) - as1
        segs.append(dict(i=i, i_prev=i_prev, rs=t, qs=q, re=te, qe=qe, bw1=int(r[4])))
        q, t, i_prev = qe, te, i
    d = dict(as1=as1, cnt1=(segs[-1]["i"] + 1 if segs else 1), rs=rs, qs=qs, T_re=t, T_qe=q, segs=segs)
    d["rs0"], d["qs0"] = (rs - int(left[3]), int(left[1])) if left is not None else (rs, qs)
    if left is not None:
        assert int(left[1] + left[2]) == qs
    d["re0"], d["qe0"] = (t + int(right[3]), q + int(right[2])) if right is not None else (t, q)
    if right is not None:
        assert int(right[1]) == q
    return d


_EXPECTED = {}


def expected(G):
    """what pga_stage_plan must return for a group, computed once per process (treat as read-only):
    dict(out (n, 21) int32 in OUT_FIELDS order, items [(m, 9) int32 per region], anchors [per query, after], regions [per region: the trace-derived
    plan, the direct wrappers' (as1, cnt1) and flags, the log])"""
    if G.name in _EXPECTED:
        return _EXPECTED[G.name]
    p = G.par()
    half_k = p["k"] >> 1
    work = [np.ascontiguousarray(a.copy()) for _, a in G.queries]
    out = np.zeros((len(G.regions), len(OUT_FIELDS)), np.int32)
    items, per_region = [], []
    for r, (j, as_, cnt) in enumerate(G.regions):
        a, q_index = work[j], G.queries[j][0]
        q = G.seqs[q_index]
        info = dict(status=0)
        per_region.append(info)
        if cnt == 0:
            out[r, 0] = info["status"] = 3
            items.append(np.zeros((0, 9), np.int32))
            continue
        ext = ref_chain_extent(len(q), a, as_, cnt)
        for f in EXTENT_FIELDS:
            out[r, OUT_FIELDS.index(f)] = ext[f]
        direct = a.copy()
        as1, cnt1 = ref_trim_and_filter(len(q), direct, as_, cnt, p)
        n_g = n_long_gaps(a, as1, cnt1)
        info.update(direct=(as1, cnt1), direct_anchors=direct, n_g=n_g, extent=ext)
        if n_g > p["g_max"]:
            out[r, 0] = info["status"] = 2                              # the kernel hands the region back untouched: no flags, nothing after r_blen
            items.append(np.zeros((0, 9), np.int32))
            continue
        log = ref_align1_trace(G, q_index, a, as_, cnt)                 # flags a
        t = parse_trace(log, a, as_, cnt, half_k, ext["rev"])
        info.update(log=log, trace=t)
        if t is None:                                                   # no DP call at all: one anchor left and no room on either side
            assert cnt1 == 1
            rs, qs = int(tpos(a)[as1]) - half_k, int(qpos(a)[as1]) - half_k
            t = dict(as1=as1, cnt1=1, rs=rs, qs=qs, rs0=rs, qs0=qs, re0=rs, qe0=qs, T_re=rs, T_qe=qs, segs=[])
        target = G.seqs[G.base + ext["rid"]]
        it = collapse(t["segs"], target, revcomp(q) if ext["rev"] else q, p)
        items.append(it)
        for f in ("as1", "cnt1", "rs", "qs", "rs0", "qs0", "re0", "qe0", "T_re", "T_qe"):
            out[r, OUT_FIELDS.index(f)] = t[f]
        out[r, OUT_FIELDS.index("n_items")] = len(it)
        out[r, OUT_FIELDS.index("n_long_gaps")] = n_g
    _EXPECTED[G.name] = dict(out=out, items=items, anchors=work, regions=per_region)
    return _EXPECTED[G.name]


# ---------------------------------------------------------------- product
def product_plan(dll, G, params=None, regions=None, queries=None):
    """pga_stage_plan -> dict(out (n, 21) int32, items [(m, 12) int32 per region], anchors [per query, after]); RuntimeError with the tap's message"""
    P = plan_params({**G.par(), **(params or {})})
    regions = G.regions if regions is None else regions
    queries = G.queries if queries is None else queries
    seqs = [np.ascontiguousarray(s, np.uint8) for s in G.seqs]
    sp = (C.c_void_p * max(1, len(seqs)))(*[s.ctypes.data for s in seqs])
    sl = np.array([len(s) for s in seqs], np.int32)
    qi = np.array([q for q, _ in queries], np.int32)
    off = np.zeros(len(queries) + 1, np.uint64)
    off[1:] = np.cumsum([len(a) for _, a in queries])
    xy = np.ascontiguousarray(np.concatenate([a.reshape(-1, 2) for _, a in queries] + [np.zeros((1, 2), np.uint64)]))
    rg = np.ascontiguousarray(np.array(regions, np.int32).reshape(-1, 3))
    out = np.zeros((len(regions), len(OUT_FIELDS)), np.int32)
    assert C.sizeof(PlanOut) == out.strides[0] if len(regions) else True
    ioff = np.zeros(len(regions) + 1, np.uint64)
    items = C.c_void_p()
    f = dll.pga_stage_plan
    f.restype = C.c_int
    f.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                  C.c_void_p, C.c_void_p, C.c_void_p]
    rc = f(len(seqs), sp, sl.ctypes.data, G.base, len(queries), qi.ctypes.data, off.ctypes.data, xy.ctypes.data, len(regions), rg.ctypes.data,
           C.addressof(P), out.ctypes.data, C.addressof(items), ioff.ctypes.data)
    if rc != 0:
        dll.pga_last_error.restype = C.c_char_p
        e = RuntimeError(dll.pga_last_error().decode())
        e.out, e.anchors = out, [xy[int(off[j]):int(off[j + 1])].copy() for j in range(len(queries))]      # as the refused call left them
        raise e
    n_items = int(ioff[-1])
    flat = np.ctypeslib.as_array(C.cast(items, C.POINTER(C.c_int32)), shape=(max(n_items, 1), 12))[:n_items].copy()
    dll.pga_free.argtypes = [C.c_void_p]
    dll.pga_free.restype = None
    dll.pga_free(items)
    return dict(out=out, items=[flat[int(ioff[r]):int(ioff[r + 1])] for r in range(len(regions))],
                anchors=[xy[int(off[j]):int(off[j + 1])].copy() for j in range(len(queries))])
