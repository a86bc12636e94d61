"""ctypes access to the post-DP stage of the three libraries (tests only).

 * reference (oracle/_ref/libmm2ref_align.so): pgref_update_extra / pgref_test_zdrop, the two wrappers of oracle/ref_align_shim.c around the
   reference's own static mm_update_extra (with mm_fix_cigar) and mm_test_zdrop.
 * restatement (oracle/libpgoracle.so): pgo_update_extra, pgo_zdrop_walk.
 * product (pangraph_amd/libpgalign.so): pga_stage_post_finish / _walk / _identity and pga_stage_zdrop_impossible (include/pga_align.h).

Sequences are numpy uint8 arrays of base codes 0..4, operation lists numpy uint32 arrays (length << 4 | op).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from pangraph_amd.mm2ffi import mm_mapopt_t
from stagebind import simple_mat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_ALIGN_SO = os.path.join(ROOT, "oracle", "_ref", "libmm2ref_align.so")

FIN_FIELDS = ("n_cigar", "qshift", "tshift", "blen", "mlen", "n_ambi", "dp_max", "n_gapo", "n_gap", "q_span", "t_span")
WALK_FIELDS = ("max_zdrop", "t0", "t1", "q0", "q1")

_REF_ALIGN = []


def ref_align_dll():
    """the shim library, built where the reference's sources are present (oracle/Makefile: ref); a skip only if oracle/_ref/ was not built"""
    if not _REF_ALIGN:
        if not os.path.exists(REF_ALIGN_SO):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True, stdout=subprocess.DEVNULL)
            if not os.path.exists(REF_ALIGN_SO):
                pytest.skip("oracle/_ref/libmm2ref_align.so not built and the reference's sources absent")
        _REF_ALIGN.append(C.CDLL(REF_ALIGN_SO))
    return _REF_ALIGN[0]


def _u8(x):
    return np.ascontiguousarray(x, dtype=np.uint8)


def revcomp(codes):
    """reverse complement of base codes; 4 stays 4"""
    c = _u8(codes)[::-1]
    return _u8(np.where(c < 4, 3 - c, 4))


def _update_extra(fn, q, t, cigar, sc):
    a, b, gq, ge = sc
    q, t = _u8(q), _u8(t)
    qp, tp = (np.concatenate([x, np.full(1, 4, np.uint8)]) for x in (q, t))       # (a squeezed-out list still reads cigar[0] and no base; never past the end)
    cg = np.ascontiguousarray(np.concatenate([np.asarray(cigar, np.uint32), np.zeros(1, np.uint32)]))
    mat = simple_mat(a, b, 1)
    out = np.zeros(7, np.int32)
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    n = fn(len(q), qp.ctypes.data, len(t), tp.ctypes.data, len(cigar), cg.ctypes.data, mat.ctypes.data, gq, ge, out.ctypes.data)
    d = dict(zip(("n_cigar", "qs", "rs", "blen", "mlen", "n_ambi", "dp_max"), (int(v) for v in out)))
    d["cigar"] = cg[:n].copy()
    return d


def ref_update_extra(q, t, cigar, sc):
    """mm_update_extra of the compiled reference on a region spanning both sequences; sc = (a, b, q, e), sc_ambi 1.
    -> dict(n_cigar, qs, rs, blen, mlen, n_ambi, dp_max, cigar)"""
    return _update_extra(ref_align_dll().pgref_update_extra, q, t, cigar, sc)


def oracle_update_extra(dll, q, t, cigar, sc):
    return _update_extra(dll.pgo_update_extra, q, t, cigar, sc)


def ref_test_zdrop(q, t, cigar, sc, zdrop, zdrop_inv=1 << 30):
    """mm_test_zdrop of the compiled reference; with zdrop_inv out of reach the inversion test is never taken: 1 iff max_zdrop > zdrop"""
    a, b, gq, ge = sc
    opt = mm_mapopt_t()
    C.memset(C.byref(opt), 0, C.sizeof(opt))
    opt.a, opt.b, opt.q, opt.e, opt.zdrop, opt.zdrop_inv, opt.max_gap = a, b, gq, ge, zdrop, zdrop_inv, 10_000
    q, t = _u8(q), _u8(t)
    cg = np.ascontiguousarray(cigar, dtype=np.uint32)
    mat = simple_mat(a, b, 1)
    fn = ref_align_dll().pgref_test_zdrop
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(mm_mapopt_t), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    return fn(C.byref(opt), q.ctypes.data, t.ctypes.data, len(cg), cg.ctypes.data, mat.ctypes.data)


def oracle_zdrop_walk(dll, q, t, cigar, sc):
    """pgo_zdrop_walk -> (max_zdrop, t0, t1, q0, q1)"""
    a, b, gq, ge = sc
    q, t = _u8(q), _u8(t)
    cg = np.ascontiguousarray(cigar, dtype=np.uint32)
    mat = simple_mat(a, b, 1)
    pos = (C.c_int * 4)()
    fn = dll.pgo_zdrop_walk
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    z = fn(q.ctypes.data, t.ctypes.data, len(cg), cg.ctypes.data, mat.ctypes.data, gq, ge, pos)
    return (z, pos[0], pos[1], pos[2], pos[3])


# ---------------------------------------------------------------- product
def _err(dll):
    dll.pga_last_error.restype = C.c_char_p
    return RuntimeError(dll.pga_last_error().decode())


def _ptrs(arrs):
    return (C.c_void_p * len(arrs))(*[x.ctypes.data for x in arrs])


def _i32(v):
    return np.ascontiguousarray(v, dtype=np.int32)


def _windows(reqs):
    """reqs: list of (forward query, q_start, q_rev, target, t_start, list)"""
    qs, ts = [_u8(r[0]) for r in reqs], [_u8(r[3]) for r in reqs]
    off = np.zeros(len(reqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(r[5]) for r in reqs])
    cg = np.ascontiguousarray(np.concatenate([np.asarray(r[5], np.uint32) for r in reqs] + [np.zeros(1, np.uint32)]))
    return (qs, ts, _ptrs(qs), _i32([len(x) for x in qs]), _i32([r[1] for r in reqs]), _i32([r[2] for r in reqs]),
            _ptrs(ts), _i32([len(x) for x in ts]), _i32([r[4] for r in reqs]), cg, off)


_POST_ARGS = [C.c_int32] + [C.c_void_p] * 9 + [C.c_int] * 5 + [C.c_void_p]


def product_post_finish(dll, reqs, sc):
    """pga_stage_post_finish.  reqs: list of (forward query, q_start, q_rev, target, t_start, list); sc = (a, b, q, e), sc_ambi 1
    -> (res (n, 11) int32 in FIN_FIELDS order, list of final lists)"""
    n = len(reqs)
    qs, ts, qp, ql, qst, qrv, tp, tl, tst, cg, off = _windows(reqs)
    res = np.zeros((n, 11), np.int32)
    a, b, gq, ge = sc
    dll.pga_stage_post_finish.restype = C.c_int
    dll.pga_stage_post_finish.argtypes = _POST_ARGS
    rc = dll.pga_stage_post_finish(n, qp, ql.ctypes.data, qst.ctypes.data, qrv.ctypes.data, tp, tl.ctypes.data, tst.ctypes.data, cg.ctypes.data, off.ctypes.data,
                                   a, b, 1, gq, ge, res.ctypes.data)
    if rc != 0:
        raise _err(dll)
    return res, [cg[int(off[i]):int(off[i]) + int(res[i, 0])].copy() for i in range(n)]


def product_post_walk(dll, reqs, sc):
    """pga_stage_post_walk -> (n, 5) int32 in WALK_FIELDS order"""
    n = len(reqs)
    qs, ts, qp, ql, qst, qrv, tp, tl, tst, cg, off = _windows(reqs)
    res = np.zeros((n, 5), np.int32)
    a, b, gq, ge = sc
    dll.pga_stage_post_walk.restype = C.c_int
    dll.pga_stage_post_walk.argtypes = _POST_ARGS
    rc = dll.pga_stage_post_walk(n, qp, ql.ctypes.data, qst.ctypes.data, qrv.ctypes.data, tp, tl.ctypes.data, tst.ctypes.data, cg.ctypes.data, off.ctypes.data,
                                 a, b, 1, gq, ge, res.ctypes.data)
    if rc != 0:
        raise _err(dll)
    return res


def product_post_identity(dll, probes, m_max):
    """pga_stage_post_identity.  probes: list of (forward query, qs on the aligned strand, q_rev, target, t_start, n) -> int32 array"""
    n = len(probes)
    qs, ts = [_u8(p[0]) for p in probes], [_u8(p[3]) for p in probes]
    ql, tl = _i32([len(x) for x in qs]), _i32([len(x) for x in ts])
    qst, qrv, tst, ln = (_i32([p[k] for p in probes]) for k in (1, 2, 4, 5))
    res = np.zeros(n, np.int32)
    dll.pga_stage_post_identity.restype = C.c_int
    dll.pga_stage_post_identity.argtypes = [C.c_int32] + [C.c_void_p] * 8 + [C.c_int, C.c_void_p]
    rc = dll.pga_stage_post_identity(n, _ptrs(qs), ql.ctypes.data, qst.ctypes.data, qrv.ctypes.data, _ptrs(ts), tl.ctypes.data, tst.ctypes.data, ln.ctypes.data,
                                     m_max, res.ctypes.data)
    if rc != 0:
        raise _err(dll)
    return res


def zdrop_impossible_fn(dll):
    """pga_stage_zdrop_impossible with its signature set once, for loops: f(q, e, q2, e2, a, zdrop, zdrop_inv, w, zdropped, score, n_cigar, address of the list)"""
    dll.pga_stage_zdrop_impossible.restype = C.c_int
    dll.pga_stage_zdrop_impossible.argtypes = [C.c_int] * 10 + [C.c_int32, C.c_void_p]
    return dll.pga_stage_zdrop_impossible


def product_zdrop_impossible(dll, q, e, q2, e2, a, zdrop, zdrop_inv, w, zdropped, score, cigar):
    """pga_stage_zdrop_impossible: host arithmetic, no device"""
    cg = np.ascontiguousarray(cigar, dtype=np.uint32)
    dll.pga_stage_zdrop_impossible.restype = C.c_int
    dll.pga_stage_zdrop_impossible.argtypes = [C.c_int] * 10 + [C.c_int32, C.c_void_p]
    return dll.pga_stage_zdrop_impossible(q, e, q2, e2, a, zdrop, zdrop_inv, w, zdropped, score, len(cg), cg.ctypes.data)


# ---------------------------------------------------------------- expected answers, computed once per process and shared (treat as read-only)
_FIN_EXPECTED = {}


def finish_expected(case, sc):
    """what pga_stage_post_finish must return for a case of tests/post_cases.py under a scoring, from the compiled reference alone:
    dict(res = the eleven PostFinRes fields, cigar = the final list, ref = the shim's answer).  n_gapo, n_gap, q_span, t_span are recomputed
    from the reference's final list, qshift / tshift are the shim's qs / rs"""
    key = (case.name, sc)
    if key not in _FIN_EXPECTED:
        r = ref_update_extra(case.q, case.t, case.cigar, sc)
        c = r["cigar"].astype(np.int64)
        op, ln = c & 0xf, c >> 4
        gap = (op == 1) | (op == 2)
        q_span = int(ln[(op == 0) | (op == 1)].sum())
        t_span = int(ln[(op == 0) | (op == 2) | (op == 3)].sum())
        res = np.array([r["n_cigar"], r["qs"], r["rs"], r["blen"], r["mlen"], r["n_ambi"], r["dp_max"], int(gap.sum()), int(ln[gap].sum()), q_span, t_span], np.int32)
        _FIN_EXPECTED[key] = dict(res=res, cigar=r["cigar"], ref=r)
    return _FIN_EXPECTED[key]
