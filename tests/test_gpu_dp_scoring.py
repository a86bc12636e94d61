"""The DP kernel classes (pga_ksw*.hip, pga_ll.hip) off the presets' scoring and on their hand-back routes, bit-exact against ksw_extd2_sse /
ksw_ll_i16 of the compiled reference, with the route counters of pga_stage_dp_routes as the proof of which kernel answered.

 (a) scorings whose gap pairs the reference EXCHANGES (ksw2_extd2_sse.c:78: q2 + e2 < q + e), an N scored as -e2 (:87, sc_ambi = 0), e == e2
     (long_thres takes its ': 0' arm), q + e == q2 + e2 (the strict '<' decides) and a = 4, through every class of dp_class;
 (b) maxima outside the 16 bits of the exact-maximum kernels' per-diagonal key (clamp16(H)): the flag, the record a clamped problem leaves,
     the second pass on the workgroup kernel (int32 H) and the splice of its results and CIGAR offsets into the first pass's (pga_ksw.hip: dp_run);
 (c) class 5, the single-wave kernel with its rows in the slab (targets wider than the workgroup kernel's LDS);
 (d) the refusal of a mismatch penalty above twice the CHEAPER pair's q + e (:100, behind the exchange).
The stage tap's windows stay forward and at offset 0."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import stagebind as sb
from pangraph_amd.synth import random_seq, mutate

pytestmark = pytest.mark.gpu

EXTZ, RIGHT, REV, APPROX, APPROX_DROP, LL = 0x40, 0x02, 0x80, 0x08, 0x10, 0x8000
UNBANDED = 150001
EXACT_KEYS = ("max", "max_q", "max_t", "mqe", "mqe_t", "mte", "mte_q")

# (a, b, sc_ambi, gapo, gape, gapo2, gape2); every one passes ksw2_extd2_sse.c:100 behind the exchange and fits int8
SCORINGS = {
    "asm10_exchanged": (1, 9, 1, 41, 1, 16, 2),
    "exchanged_N_is_e2": (2, 4, 0, 24, 1, 4, 2),
    "N_is_e2": (1, 9, 0, 16, 2, 41, 1),
    "e_equals_e2": (1, 4, 1, 6, 2, 26, 2),
    "equal_open_cost": (1, 9, 1, 16, 2, 17, 1),
    "a_is_4": (4, 8, 2, 12, 4, 48, 2),
}


def _nt4(s):
    return sb.nt4(np.asarray(s, dtype=np.uint8).tobytes().decode())


def _n_run(rng, s, k=None):
    s = s.copy()
    if len(s) > 8:
        k = min(k or int(rng.integers(2, 9)), len(s) // 2)
        p = int(rng.integers(0, len(s) - k + 1))
        s[p:p + k] = ord("N")
    return s


def _indel(rng, q, lo=20, hi=61, kind=None):
    """one insertion or deletion of lo ... hi - 1 bases inside q"""
    k = int(rng.integers(lo, hi))
    p = int(rng.integers(len(q) // 4, 3 * len(q) // 4 + 1))
    if (int(rng.integers(0, 2)) if kind is None else kind) == 0 or len(q) < 2 * k + 8:
        return np.concatenate([q[:p], random_seq(rng, k), q[p:]])
    return np.concatenate([q[:p], q[p + k:]])


def _set_routing(monkeypatch, pipe=None, bstrips=None, lb=None):
    for k_, v_ in (("PGA_PIPE", pipe), ("PGA_BSTRIPS", bstrips), ("PGA_LB", lb)):
        if v_ is None:
            monkeypatch.delenv(k_, raising=False)
        else:
            monkeypatch.setenv(k_, v_)


def _check(tag, jobs, got, exp):
    for i, (j, g, e) in enumerate(zip(jobs, got, exp)):
        where = (tag, i, len(j[0]), len(j[1]), j[2], j[3], j[4], hex(j[5]))
        if j[5] & LL:
            assert (g["score"], g["max_q"], g["max_t"]) == e, where + ((g["score"], g["max_q"], g["max_t"]), e)
            continue
        for k in ("zdropped", "reach_end", "cigar", "score") + (() if j[5] & APPROX else EXACT_KEYS):
            assert g[k] == e[k], where + (k, g[k] if k != "cigar" else len(g[k]), e[k] if k != "cigar" else len(e[k]))


def _reference(ref_lib, jobs, sc):
    a, b, amb, q1, e1, q2, e2 = sc
    mat = sb.simple_mat(a, b, amb)
    return [sb.ref_ll(ref_lib.dll, qn, tn, mat, q1, e1) if fl & LL else sb.ref_extd2(ref_lib.dll, qn, tn, mat, q1, e1, q2, e2, w, zd, eb, fl)
            for (qn, tn, w, zd, eb, fl) in jobs]


# ---------------------------------------------------------------- (a) the scoring sweep
@functools.lru_cache(maxsize=None)
def _sweep_jobs():
    """~70 problems, at least one in every class of dp_class (pga_ksw.hip), at the smallest shapes that reach it; the sequences do not depend on
    the scoring.  About a third carry an N run, about a third an indel of 20 ... 60 bases (both gap kinds and their ties)."""
    rng = np.random.default_rng(20261017)
    jobs, n = [], [0]

    def add(q, t, w, zd, eb, fl, deco=True, keep_len=False):
        i = n[0]; n[0] += 1
        if deco and (i % 3 == 0 or i % 11 == 5):
            if i % 9 != 3:
                q = _n_run(rng, q)
            if i % 9 != 0:
                t = _n_run(rng, t)
        if deco and i % 3 == 1 and not keep_len and len(q) >= 120:
            q = _indel(rng, q)
        jobs.append((_nt4(q), _nt4(t), w, zd, eb if fl & EXTZ else -1, fl))

    # classes 0 and 1 (register tiles, pga_ksw_fast.hip): the band never binds, target <= 256 / <= 512.  An approximate fill whose lengths differ by
    # <= 12 would go to the corridor kernel (class 8): those of this block get an insertion of 20 ... 60 bases
    for tl in (1, 17, 256, 257, 512):
        for fl in (APPROX, 0, EXTZ):
            t = random_seq(rng, tl)
            q = mutate(rng, t, snp=0.05, indel=0.004 if tl > 30 else 0.0)
            if fl == APPROX:
                q = np.concatenate([q[: len(q) // 2], random_seq(rng, int(rng.integers(20, 61))), q[len(q) // 2:]])
            add(q, t, UNBANDED, (200, 400)[tl % 2], (-1, 10)[tl % 2], fl, keep_len=(fl == APPROX))
    # class 8 (the corridor, pga_ksw_band.hip): flag exactly KSW_EZ_APPROX_MAX, unbanded, |qlen - tlen| <= 12, lengths <= 1024
    for L in (1, 2, 31, 33, 300, 1024):
        t = random_seq(rng, L)
        add(t.copy(), t, UNBANDED, 200, -1, APPROX, deco=False)                                       # clean
        if L >= 31:
            add(mutate(rng, t, snp=0.1, indel=0.0), t, UNBANDED, 200, -1, APPROX, deco=False)          # diverged
            add(_n_run(rng, mutate(rng, t, snp=0.02, indel=0.0), 6), _n_run(rng, t, 3), UNBANDED, 200, -1, APPROX, deco=False)
        if L >= 300:                                                                                  # an insertion here, a deletion there
            k = int(rng.integers(20, 55)); d = k + int(rng.integers(0, 7))
            q = np.concatenate([t[:L // 3], random_seq(rng, k), t[L // 3:]])
            p = 2 * L // 3
            add(np.concatenate([q[:p], q[p + d:]]), t, UNBANDED, 200, -1, APPROX, deco=False)
    # classes 11 and 10 (lane kernels, pga_ksw_lanes.hip): the band ring (min(w, tlen) rounded to 16, + 96) fits 512 / 2 048 columns.  The exact
    # ones go on to the workgroup pipeline (13) and the banded wave strips (12) by the launch's composition and the two switches
    flags = (EXTZ, EXTZ | RIGHT | REV, 0, RIGHT, APPROX, APPROX | APPROX_DROP)
    for wi, (w, Ls) in enumerate(((64, (600, 1100)), (257, (700, 1300)), (751, (900, 1700)), (1501, (1700, 2500)))):
        for fi, fl in enumerate(flags):
            L = Ls[(fi + wi) % 2]
            t = random_seq(rng, L)
            q = mutate(rng, t, snp=0.01 * (1 + fi % 4), indel=0.002)
            if (fi + wi) % 3 == 0 and fl & EXTZ:                                                       # homology ends: the z-drop decides
                cut = int(rng.integers(100, L // 2)); q = np.concatenate([q[:cut], random_seq(rng, L - cut)])
            add(q, t, w, (100, 400, -1)[(fi + wi) % 3], (-1, 10)[fi % 2], fl)
    # the length-bound stop (pga_dp.h): target windows of <= 64 bases, the query running on past w + 2 tlen
    k_of = (0, 5, 300, 1)
    for ti, tl in enumerate((1, 16, 33, 64)):
        for wi, w in enumerate((64, 1501)):
            t = random_seq(rng, tl)
            ql = w + 2 * tl + k_of[(ti + wi) % 4]
            head = mutate(rng, t, snp=0.08 * (ti % 2), indel=0.0)
            body = random_seq(rng, ql - len(head))
            if ti % 2 == 1:                                                                           # the window again, far from the diagonal
                for p in range(40, len(body) - tl - 1, max(tl + 3, 97)):
                    body[p:p + tl] = t
            add(np.concatenate([head, body]), t, w, (200, 400, 100, -1)[(ti + wi) % 4], (-1, 10)[wi], (EXTZ, EXTZ | RIGHT | REV, 0, EXTZ | REV)[(ti + 2 * wi) % 4], deco=(tl >= 33), keep_len=True)
    # class 9 (wave strips, pga_ksw_wstrips.hip): unbanded, qlen >= 256, target >= 1 536 (approximate) / >= 2 048 (exact)
    for fl in (APPROX, 0):
        t = random_seq(rng, 2100)
        add(mutate(rng, t, snp=0.03, indel=0.003), t, UNBANDED, 400, -1, fl)
    # classes 2, 3 or 7 (workgroup kernel, pga_ksw_wide.hip): a ring of 2 976 columns is beyond the lane kernels
    t = random_seq(rng, 3000)
    add(mutate(rng, t, snp=0.02, indel=0.002), t, 2873, 400, 10, EXTZ)
    # class 6 (pga_ll.hip): ksw_ll_i16 with the scoring's first pair as given
    for (lq, lt) in ((1, 1), (37, 250), (900, 640), (333, 899)):
        t = random_seq(rng, lt); q = random_seq(rng, lq)
        if min(lq, lt) > 30:
            L = min(lq, lt) // 2
            piece = mutate(rng, t[lt // 4: lt // 4 + L], snp=0.05, indel=0.01)[:L]
            q[lq // 3: lq // 3 + len(piece)] = piece[: lq - lq // 3]
        add(q, t, 0, 0, -1, LL, deco=(lq == 900))
    return tuple(jobs)


@pytest.mark.parametrize("name", list(SCORINGS))
def test_every_dp_class_under_scorings_off_the_presets_vs_reference(gpu_lib, ref_lib, monkeypatch, name):
    """One job list through default routing, PGA_PIPE=force, PGA_BSTRIPS=force, both switched off (the lane kernels keep their exact problems: with
    a list this small the default hands all of them to the pipeline and the wave strips) and PGA_LB=check (the problems the length-bound stop
    covers stay with the lane kernel, which sweeps on and fails the call if the record changes).  The route counters say which classes ran."""
    sc = SCORINGS[name]
    a, b, amb, q1, e1, q2, e2 = sc
    jobs = list(_sweep_jobs())
    assert 60 <= len(jobs) <= 80
    exp = _reference(ref_lib, jobs, sc)
    ext = [e for j, e in zip(jobs, exp) if not j[5] & LL]
    assert sum(e["zdropped"] for e in ext) >= 4 and sum(e["reach_end"] for e in ext) >= 1 and sum(1 for e in ext if len(e["cigar"]) >= 3) >= 20
    sb.product_dp_routes(gpu_lib.dll)
    for tag, env in (("default", {}), ("pipe", dict(pipe="force")), ("bstrips", dict(bstrips="force")), ("lanes", dict(pipe="off", bstrips="off")), ("lb_check", dict(lb="check"))):
        _set_routing(monkeypatch, **env)
        got = sb.product_extd2(gpu_lib.dll, jobs, a, b, amb, q1, e1, q2, e2)
        by_class, back = sb.product_dp_routes(gpu_lib.dll)
        print(name, tag, "by_class", by_class, "handed_back", back)
        _check((name, tag), jobs, got, exp)
        if tag in ("default", "lb_check"):
            for c in (0, 1, 6, 8, 9, 10, 11):
                assert by_class[c] >= 1, (name, tag, c, by_class)
            assert by_class[2] + by_class[3] + by_class[7] >= 1, (name, tag, by_class)
        if tag == "pipe":
            assert by_class[13] >= 1, (name, tag, by_class)
        if tag == "bstrips":
            assert by_class[12] >= 1, (name, tag, by_class)
        if tag == "lanes":
            assert by_class[12] == 0 and by_class[13] == 0 and by_class[10] >= 12 and by_class[11] >= 12, (name, tag, by_class)


# ---------------------------------------------------------------- (b) the 16-bit clamp and its hand-back
# the four ways a banded exact problem is answered: what the launch's composition picks (for lists this small: the banded wave strips), the
# workgroup pipeline, the banded wave strips, the lane kernel
BANDED_ROUTES = (("default", {}, None), ("pipe", dict(pipe="force"), 13), ("bstrips", dict(pipe="off", bstrips="force"), 12), ("lanes", dict(pipe="off", bstrips="off"), None))


@pytest.mark.parametrize("w", (64, 751))
def test_clamp_boundary_32766_stays_32768_is_handed_back(gpu_lib, ref_lib, monkeypatch, w):
    """identical windows of 16 383 and 16 384 bases at a = 2: the reference's max is 32 766 (the largest the key holds unclamped) and 32 768.
    Exactly one of the two (and neither of the two short-lived problems beside them) is handed back (-9), by the one-wave (w = 64) and the four-wave (w = 751) lane kernel, the pipeline and the banded wave
    strips alike, and both records are the reference's."""
    sc = (2, 4, 1, 4, 2, 24, 1)
    a, b, amb, q1, e1, q2, e2 = sc
    rng = np.random.default_rng(16384)
    s = random_seq(rng, 16384)
    jobs = [(_nt4(s[:L]), _nt4(s[:L]), w, 400, -1, EXTZ) for L in (16383, 16384)]
    # Two more problems whose homology ends after 150 bases: they z-drop early, and the direction-matrix chunks the lane kernel's pool holds for
    # their 28 000 nominal bases keep it from running dry under the pair, which sweeps every diagonal (a dry pool hands back as well).  The pool
    # holds every problem's nominal need, 69 chunks at w = 751; the workgroup with the smallest share may take the 44th; the four problems ask
    # for 14 + 14 + 3 + 3 (lanes_pool_chunks in pga_ksw.hip, want_chunk in pga_ksw_lanes.hip)
    for _ in range(2):
        t = random_seq(rng, 28000)
        jobs.append((_nt4(np.concatenate([t[:150], random_seq(rng, 27850)])), _nt4(t), w, 400, -1, EXTZ))
    exp = _reference(ref_lib, jobs, sc)
    assert [e["max"] for e in exp[:2]] == [32766, 32768] and all(e["max"] < 400 and e["zdropped"] for e in exp[2:])
    lane_class = 11 if w == 64 else 10
    sb.product_dp_routes(gpu_lib.dll)
    for tag, env, cls in BANDED_ROUTES:
        _set_routing(monkeypatch, **env)
        got = sb.product_extd2(gpu_lib.dll, jobs, a, b, amb, q1, e1, q2, e2)
        by_class, back = sb.product_dp_routes(gpu_lib.dll)
        print(w, tag, "by_class", by_class, "handed_back", back)
        _check((w, tag), jobs, got, exp)
        assert back[1] == 1, (w, tag, by_class, back)
        if tag == "lanes":
            assert by_class[lane_class] == 4, (w, tag, by_class)
        elif cls is not None:
            assert by_class[cls] == 4, (w, tag, by_class)


@pytest.mark.parametrize("w", (64, 751))
def test_clamp_inside_a_mixed_banded_launch_is_spliced_back(gpu_lib, ref_lib, monkeypatch, w):
    """a = 4: 8 400 bases at 0.2 % substitutions pass 32 767 mid-sweep.  Two such problems (a left extension and a banded global fill) sit among
    a dozen short ones of the same class; the two come back from the workgroup kernel and are spliced into the first pass's records, their CIGARs
    behind the first pass's pool (dp_run: res[redo[k]].cigar_off += base)."""
    sc = SCORINGS["a_is_4"]
    a, b, amb, q1, e1, q2, e2 = sc
    rng = np.random.default_rng(8400 + w)
    jobs = []
    for i in range(14):
        fl = (EXTZ | RIGHT | REV, 0)[i % 2]
        if i in (6, 9):
            t = random_seq(rng, 8400)
            q = mutate(rng, t, snp=0.002, indel=0.0)
        else:
            L = int(rng.integers(150, 500)) if w == 64 else int(rng.integers(800, 1100))     # (the ring of the short ones is their class's too)
            t = random_seq(rng, L)
            q = mutate(rng, t, snp=0.03, indel=0.004)
            if i % 5 == 2:
                q = _indel(rng, q)
        jobs.append((_nt4(q), _nt4(t), w, 400, -1, fl))
    exp = _reference(ref_lib, jobs, sc)
    assert all((e["max"] >= 32768) == (i in (6, 9)) for i, e in enumerate(exp)) and not exp[6]["zdropped"] and not exp[9]["zdropped"]
    sb.product_dp_routes(gpu_lib.dll)
    for tag, env, cls in BANDED_ROUTES:
        _set_routing(monkeypatch, **env)
        got = sb.product_extd2(gpu_lib.dll, jobs, a, b, amb, q1, e1, q2, e2)
        by_class, back = sb.product_dp_routes(gpu_lib.dll)
        print(w, tag, "by_class", by_class, "handed_back", back)
        _check((w, tag), jobs, got, exp)
        assert back[1] == 2, (w, tag, by_class, back)
        if tag == "lanes":
            assert by_class[11 if w == 64 else 10] == 14, (w, tag, by_class)
        elif cls is not None:
            assert by_class[cls] >= 2, (w, tag, by_class)


def test_clamp_in_exact_wave_strips_is_spliced_back(gpu_lib, ref_lib, monkeypatch):
    """the same 8 400 x 8 400 problem unbanded with flag 0: wave strips in exact mode (class 9), redone by the workgroup kernel, among strips
    problems that stay"""
    sc = SCORINGS["a_is_4"]
    a, b, amb, q1, e1, q2, e2 = sc
    rng = np.random.default_rng(84008400)
    jobs = []
    for L, fl, snp in ((2100, 0, 0.03), (300, 0, 0.05), (8400, 0, 0.002), (2100, APPROX, 0.03), (700, EXTZ, 0.03)):
        t = random_seq(rng, L)
        jobs.append((_nt4(mutate(rng, t, snp=snp, indel=0.002 if L < 8400 else 0.0)), _nt4(t), UNBANDED, 400, -1, fl))
    exp = _reference(ref_lib, jobs, sc)
    assert exp[2]["max"] >= 32768 and not exp[2]["zdropped"] and max(e["max"] for i, e in enumerate(exp) if i != 2) < 32767
    _set_routing(monkeypatch)
    sb.product_dp_routes(gpu_lib.dll)
    got = sb.product_extd2(gpu_lib.dll, jobs, a, b, amb, q1, e1, q2, e2)
    by_class, back = sb.product_dp_routes(gpu_lib.dll)
    print("by_class", by_class, "handed_back", back)
    _check("wstrips", jobs, got, exp)
    assert by_class[9] == 3 and back[1] == 1, (by_class, back)


def test_negative_clamp_of_a_global_fill_through_unrelated_sequence(gpu_lib, ref_lib, monkeypatch):
    """asm5, flag 0, no z-drop, w = 64, unrelated windows of 11 000 bases (a 64-column band through unrelated sequence loses 3.13 per base under asm5:
    9 000 bases end at -28 183, inside the key): the reference's score is below -32 768, so the only cell of the last diagonal clamps at the key's
    lower end and the problem is handed back -- by the kernel the default picks and by the lane kernel"""
    sc = (1, 19, 1, 39, 3, 81, 1)
    a, b, amb, q1, e1, q2, e2 = sc
    rng = np.random.default_rng(11000)
    jobs = [(_nt4(random_seq(rng, L)), _nt4(random_seq(rng, L)), 64, -1, -1, 0) for L in (300, 11000, 450)]
    exp = _reference(ref_lib, jobs, sc)
    assert exp[1]["score"] <= -32768 and exp[0]["score"] > -32767 and exp[2]["score"] > -32767
    sb.product_dp_routes(gpu_lib.dll)
    for tag, env in (("default", {}), ("lanes", dict(pipe="off", bstrips="off"))):
        _set_routing(monkeypatch, **env)
        got = sb.product_extd2(gpu_lib.dll, jobs, a, b, amb, q1, e1, q2, e2)
        by_class, back = sb.product_dp_routes(gpu_lib.dll)
        print(tag, "by_class", by_class, "handed_back", back)
        _check(tag, jobs, got, exp)
        assert back[1] >= 1, (tag, by_class, back)
        if tag == "lanes":
            assert by_class[11] == 3, (tag, by_class)


# ---------------------------------------------------------------- (c) class 5
@pytest.mark.parametrize("name", ("asm10", "exchanged_N_is_e2"))
def test_single_wave_kernel_with_rows_in_the_slab_vs_reference(gpu_lib, ref_lib, monkeypatch, name):
    """k_extd2 (pga_ksw.hip), the last resort of dp_class: an unbanded target of 11 300 bases needs 14 x 11 312 B of ring, more than the workgroup
    kernel's LDS; a query of >= 256 bases with flag 0 would go to the wave strips, so the global fill has 200"""
    sc = (1, 9, 1, 16, 2, 41, 1) if name == "asm10" else SCORINGS[name]
    a, b, amb, q1, e1, q2, e2 = sc
    rng = np.random.default_rng(11300)
    t = random_seq(rng, 11300)
    jobs = []
    for i, (ql, fl) in enumerate(((200, EXTZ), (300, EXTZ), (200, EXTZ | RIGHT | REV), (300, EXTZ | RIGHT | REV), (200, 0))):
        q = mutate(rng, t[:ql + 40], snp=0.04, indel=0.01)[:ql]
        assert len(q) == ql
        if i == 3:
            q = _n_run(rng, q, 7)
        if i == 1:
            q = _indel(rng, q, 20, 40, kind=0)[:ql]
        jobs.append((_nt4(q), _nt4(t), UNBANDED, 400 if fl else -1, (-1, 10)[i % 2], fl))
    exp = _reference(ref_lib, jobs, sc)
    _set_routing(monkeypatch)
    sb.product_dp_routes(gpu_lib.dll)
    got = sb.product_extd2(gpu_lib.dll, jobs, a, b, amb, q1, e1, q2, e2)
    by_class, back = sb.product_dp_routes(gpu_lib.dll)
    print(name, "by_class", by_class, "handed_back", back)
    _check(name, jobs, got, exp)
    assert by_class[5] == len(jobs) and sum(by_class) == len(jobs) and back == [0, 0], (by_class, back)


# ---------------------------------------------------------------- (d) the refusal
def test_mismatch_penalty_above_twice_the_cheaper_gap_pair_is_refused_by_name(gpu_lib):
    """ksw2_extd2_sse.c:100 tests -min_sc > 2 (q + e) BEHIND the exchange of the pairs (:78), i.e. against the cheaper one, and returns an empty record
    for every problem: an option set with b = 40 and the pairs (41, 1), (16, 2) -- above 2 x 18, not above 2 x 42 -- is refused when the batch starts,
    naming the option, in either order of the pairs."""
    rng = np.random.default_rng(13)
    seqs = [random_seq(rng, 3000).tobytes().decode() for _ in range(2)]
    old = os.environ.get("PGA_MM_MAP_SOFT_ERRORS")
    os.environ["PGA_MM_MAP_SOFT_ERRORS"] = "1"
    try:
        for (q1, e1, q2, e2) in ((41, 1, 16, 2), (16, 2, 41, 1)):
            io, mo = gpu_lib.make_options("asm10", c=True, X=True, s=90, bucket_bits=14)
            mo.b, mo.q, mo.e, mo.q2, mo.e2 = 40, q1, e1, q2, e2
            idx = gpu_lib.index(seqs, ["1", "2"], io, mo)
            try:
                assert idx.map(seqs[0], "1") == []
                gpu_lib.dll.pga_last_error.restype = C.c_char_p
                msg = gpu_lib.dll.pga_last_error().decode()
                assert "b = 40" in msg and "2*(q+e) = 36" in msg, ((q1, e1, q2, e2), msg)
            finally:
                idx.close()
    finally:
        if old is None:
            del os.environ["PGA_MM_MAP_SOFT_ERRORS"]
        else:
            os.environ["PGA_MM_MAP_SOFT_ERRORS"] = old
