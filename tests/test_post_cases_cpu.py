"""The cases of tests/post_cases.py on the CPU.  Every finish case goes through the reference's own mm_update_extra (oracle/ref_align_shim.c) and
every pin -- the property a case was built for -- is asserted from that answer alone: a case whose pin does not hold is a broken generator.  The
restatement's pgo_update_extra must agree with the reference field for field and list for list; pgo_zdrop_walk, the authority of the GPU test for
the walk, is pinned on the reference's mm_test_zdrop by bracketing and on a vectorised recomputation of the tracker; and the host shortcut
zdrop_impossible (pga_stage_zdrop_impossible: host arithmetic, the product library loads without a device) may only say "skip the walk" where the
walk would have found nothing."""
import ctypes as C
import struct

import numpy as np
import pytest

import post_cases as pc
import postbind as pb

CASES = pc.all_cases()
POOL_A, POOL_B = pc.batch_pools()
EVERY = CASES + POOL_A + POOL_B
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in pc.FAMILIES}


def test_generators_are_deterministic_and_well_formed():
    again = {c.name: c for c in pc.all_cases()}
    assert len(again) == len(CASES), "case names are unique"
    assert set(c.family for c in CASES) == set(pc.FAMILIES)
    for c in EVERY:
        assert c.t.dtype == np.uint8 and c.q.dtype == np.uint8 and c.cigar.dtype == np.uint32, c.name
        assert pc.spans(c.cigar) == (len(c.q), len(c.t)), f"{c.name}: the list spans both sequences"
        assert (c.cigar & 0xf).max() <= 3 and (len(c.t) == 0 or c.t.max() <= 4) and (len(c.q) == 0 or c.q.max() <= 4), c.name
        assert len(c.q) + len(c.t) <= 25_000, c.name
    for c in CASES:
        d = again[c.name]
        assert np.array_equal(c.t, d.t) and np.array_equal(c.q, d.q) and np.array_equal(c.cigar, d.cigar), c.name
    assert sum(1 for c in BY_FAMILY["random"] if (c.cigar & 0xf == 3).any()) >= 20, "some random lists hold operation 3"
    assert len(BY_FAMILY["random"]) >= 200


def test_batches_reuse_waves_with_other_and_longer_lists():
    b = pc.batches()
    assert len(b["batch_4097"]) == 4097 and len(b["batch_8200"]) == 8200
    big = b["batch_8200"]
    first = set(c.name for c in big[:8192])
    for j, c in enumerate(big[8192:]):
        assert c.name not in first, "requests beyond 8192 differ from the first 8192"
        assert len(c.cigar) > len(big[j].cigar), "... and bring a longer list than their predecessor on the same wave"


def mg_log2(x):
    """mmpriv.h:118-126 in float32 arithmetic"""
    f32 = np.float32
    z = struct.unpack("<I", struct.pack("<f", x))[0]
    r = f32(((z >> 23) & 255) - 128)
    z = (z & ~(255 << 23) & 0xffffffff) + (127 << 23)
    f = f32(struct.unpack("<f", struct.pack("<I", z))[0])
    return float(f32(r + f32(f32(f32(f32(f32(-0.34484843) * f) + f32(2.02466578)) * f) - f32(0.67487759))))


def stepwise(q, t, cigar, sc):
    """the running score of mm_update_extra (align.c:250-286), base by base -> (dp_max, s was positive and hit the clamp inside a match run,
    s entered a match run with a fractional part)"""
    a, b, gq, ge = sc
    q, t = q.tolist(), t.tolist()
    s = mx = 0.0
    i = j = 0
    zero = frac = False
    for x in cigar.tolist():
        op, ln = x & 0xf, x >> 4
        if op == 0:
            frac |= ln > 0 and s != int(s)
            for l in range(ln):
                cq, ct = q[j + l], t[i + l]
                was = s
                s += -1 if cq > 3 or ct > 3 else a if cq == ct else -b
                if s < 0:
                    s = 0.0
                    zero |= was > 0
                else:
                    mx = max(mx, s)
            i += ln; j += ln
        elif op in (1, 2):
            s = max(0.0, s - (gq + float(ge) * mg_log2(1.0 + ln)))
            if op == 1: j += ln
            else: i += ln
        else:
            i += ln
    return int(mx + .499), zero, frac


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_pins_hold_on_the_reference(family):
    n_pins = 0
    for c in BY_FAMILY[family]:
        r = pb.finish_expected(c, pc.PIN_SC)["ref"]
        p, fin = c.pins, r["cigar"]
        assert r["n_cigar"] == len(fin)
        if "final" in p:
            assert pc.cigstr(fin) == p["final"], f"{c.name}: {pc.cigstr(c.cigar)} came back as {pc.cigstr(fin)}"
        for k in ("qs", "rs"):
            if k in p:
                assert r[k] == p[k], (c.name, k, r[k])
        if "n_final" in p:
            assert r["n_cigar"] == p["n_final"], (c.name, r["n_cigar"])
        if "n_final_gt" in p:
            assert r["n_cigar"] > p["n_final_gt"], (c.name, r["n_cigar"])
        if p.get("squeezed"):
            assert r["n_cigar"] < len(c.cigar) and (fin >> 4).min() > 0, c.name
        if p.get("n_ambi"):
            assert r["n_ambi"] > 0, c.name
        dp_max, zero, frac = stepwise(c.q[r["qs"]:], c.t[r["rs"]:], fin, pc.PIN_SC)
        assert dp_max == r["dp_max"], f"{c.name}: the stepwise loop gives {dp_max}, the reference {r['dp_max']}"
        if "dp_max" in p:
            assert r["dp_max"] == p["dp_max"], (c.name, r["dp_max"])
        if p.get("s_zero"):
            assert zero, f"{c.name}: s never falls back to zero inside a run"
        if p.get("frac"):
            assert frac, f"{c.name}: s is whole at the start of every run"
        n_pins += len(p)
    assert n_pins > 0 or family == "random"


def test_family_pins_cover_what_they_were_built_for():
    """the counts behind the families: slide lengths on both sides of a ballot with and without slid == room, both list routes"""
    s = [c for c in BY_FAMILY["slides"]]
    for k in pc.SLIDES:
        for kind in "ID":
            assert sum(1 for c in s if c.name.startswith(f"slide_{kind}_") and c.name.endswith(f"_{k}_stop")) == 3
            assert sum(1 for c in s if c.name.startswith(f"slide_{kind}_") and c.name.endswith(f"_{k}_room")) == 3
    fin = {c.name: (len(c.cigar), pb.finish_expected(c, pc.PIN_SC)["ref"]["n_cigar"], pb.finish_expected(c, pc.PIN_SC)["ref"]["qs"]) for c in BY_FAMILY["long_lists"]}
    assert sorted(v[1] for k, v in fin.items() if "random" not in k) == [6143, 6143, 6144, 6144, 6145, 6145, 7001, 7001]
    assert any(n_in > pc.FIN_LDS_OPS and qs > 0 for n_in, _, qs in fin.values()), "the in-HBM route with a leading indel"
    assert any(n_in == pc.FIN_LDS_OPS and qs > 0 for n_in, _, qs in fin.values()), "the fullest LDS list with a leading indel"
    assert any(n_in == pc.FIN_LDS_OPS + 1 and qs == 0 for n_in, _, qs in fin.values())


@pytest.mark.parametrize("sc", pc.SCORINGS, ids=[str(s) for s in pc.SCORINGS])
def test_restatement_update_extra_vs_reference(sc, oracle_lib):
    for c in EVERY:
        r = pb.finish_expected(c, sc)["ref"]
        o = pb.oracle_update_extra(oracle_lib.dll, c.q, c.t, c.cigar, sc)
        for k in ("n_cigar", "qs", "rs", "blen", "mlen", "n_ambi", "dp_max"):
            assert o[k] == r[k], f"{c.name}: {k} restatement {o[k]}, reference {r[k]}"
        assert np.array_equal(o["cigar"], r["cigar"]), f"{c.name}: {pc.cigstr(o['cigar'])} vs {pc.cigstr(r['cigar'])}"


def walk_numpy(q, t, cigar, sc):
    """the tracker of mm_test_zdrop (align.c:32-68) over prefix scores, vectorised -> (max_zdrop, t0, t1, q0, q1)"""
    a, b, gq, ge = sc
    inc, ti, qj = [], [], []
    i = j = 0
    for x in cigar.tolist():
        op, ln = x & 0xf, x >> 4
        if op == 0:
            tt, qq = t[i:i + ln], q[j:j + ln]
            inc.append(np.where((tt > 3) | (qq > 3), -1, np.where(tt == qq, a, -b)).astype(np.int64))
            ti.append(np.arange(i, i + ln)); qj.append(np.arange(j, j + ln))
            i += ln; j += ln
        else:
            if op == 1: j += ln
            else: i += ln
            inc.append(np.array([-(gq + ge * ln)], np.int64)); ti.append(np.array([i])); qj.append(np.array([j]))
    inc, ti, qj = (np.concatenate(v) for v in (inc, ti, qj))
    if len(inc) == 0:
        return (0, -1, -1, -1, -1)
    cum = np.cumsum(inc)
    before = np.concatenate([[np.iinfo(np.int64).min], np.maximum.accumulate(cum)[:-1]])      # the best prefix score in front of each step
    rec = cum >= before                                                                        # steps that set a new best (ties move it on)
    last = np.maximum.accumulate(np.where(rec, np.arange(len(cum)), -1))
    bi = np.concatenate([[0], last[:-1]])                                                      # the best prefix each step is compared with
    z = np.where(rec, 0, cum[bi] - cum - np.abs((ti - ti[bi]) - (qj - qj[bi])) * ge)
    e = int(np.argmax(z))
    if z[e] <= 0:
        return (0, -1, -1, -1, -1)
    return (int(z[e]), int(ti[bi[e]]), int(ti[e]), int(qj[bi[e]]), int(qj[e]))


@pytest.mark.parametrize("sc", pc.SCORINGS, ids=[str(s) for s in pc.SCORINGS])
def test_restatement_walk_vs_reference(sc, oracle_lib):
    n_pos = 0
    for c in EVERY:
        w = pb.oracle_zdrop_walk(oracle_lib.dll, c.q, c.t, c.cigar, sc)
        z = w[0]
        assert z >= 0
        assert pb.ref_test_zdrop(c.q, c.t, c.cigar, sc, z) == 0, f"{c.name}: mm_test_zdrop at zdrop = max_zdrop = {z}"
        if z > 0:
            assert pb.ref_test_zdrop(c.q, c.t, c.cigar, sc, z - 1) == 1, f"{c.name}: mm_test_zdrop at zdrop = max_zdrop - 1 = {z - 1}"
            n_pos += 1
        assert w == walk_numpy(c.q, c.t, c.cigar, sc), f"{c.name}: the window does not give max_zdrop from the prefix scores"
    assert n_pos >= 200


ZDROPS = ((200, 200), (400, 200), (100, 25), (2000, 1500))     # (zdrop, zdrop_inv): the asm presets', minimap2's default, a tight and a loose pair
UNITS = (0, 1, 2, 5)


def path_score(c, sc):
    """(the list's own score under the dual gap costs, its match columns that do not hold a match)"""
    a, b, gq, ge = sc
    q2, e2 = pc.DUAL[sc]
    s = i = j = nonmatch = 0
    for x in c.cigar.tolist():
        op, ln = x & 0xf, x >> 4
        if op == 0:
            tt, qq = c.t[i:i + ln], c.q[j:j + ln]
            s += int(np.where((tt > 3) | (qq > 3), -1, np.where(tt == qq, a, -b)).sum())
            nonmatch += int(((tt > 3) | (qq > 3) | (tt != qq)).sum())
            i += ln; j += ln
        else:
            s -= min(gq + ge * ln, q2 + e2 * ln)
            if op == 1: j += ln
            else: i += ln
    return s, nonmatch


def least_limit(tap, gq, ge, q2, e2, a, w, score, n_cg, p_cg):
    """the smallest zdrop = zdrop_inv at which the shortcut says "skip" (its own bound on the walk, found by bisection), None if it never does"""
    lo, hi = -1, 1 << 30
    if not tap(gq, ge, q2, e2, a, hi, hi, w, 0, score, n_cg, p_cg):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if tap(gq, ge, q2, e2, a, mid, mid, w, 0, score, n_cg, p_cg):
            hi = mid
        else:
            lo = mid
    return hi


def test_zdrop_impossible_only_skips_walks_that_find_nothing(product_so, oracle_lib):
    """Every list with its own path score under the dual gap costs, as the answer of a pass whose band covers the matrix: whenever the shortcut
    says "skip", the walk finds at most min(zdrop, zdrop_inv).

    The score plus a few units.  The shortcut bounds the walk by a * L - score - (cheapest gap costs) + (the walk's gap costs), which overstates
    the true sum of decrements along the path by a per match column that holds no match.  A score above the path's own therefore stays inside
    the proof up to a * (such columns), and the units 1, 2 and 5 are tried wherever they are within that margin.  Beyond it no test that sees no
    base can hold: run_300_burst_10_3 under (1, 9, 16, 2) at its path score 270 + 5, with three mismatches, is answered "skip" for
    min(zdrop, zdrop_inv) = 25 while the walk finds 27.  Where such pairs really come from -- a pass whose band cuts the matrix -- and that the
    shortcut refuses them is the subject of test_zdrop_impossible_on_the_reference_dp."""
    tap = pb.zdrop_impossible_fn(C.CDLL(product_so))
    n_true = n_false = n_units = 0
    for sc in pc.SCORINGS:
        a, b, gq, ge = sc
        q2, e2 = pc.DUAL[sc]
        for c in EVERY:
            z = pb.oracle_zdrop_walk(oracle_lib.dll, c.q, c.t, c.cigar, sc)[0]
            ps, nonmatch = path_score(c, sc)
            cg = np.ascontiguousarray(c.cigar)
            n_cg, p_cg, w = len(cg), cg.ctypes.data, max(len(c.q), len(c.t))
            for zdrop, zdrop_inv in ZDROPS:
                for u in UNITS:
                    if u > a * nonmatch:
                        continue
                    if tap(gq, ge, q2, e2, a, zdrop, zdrop_inv, w, 0, ps + u, n_cg, p_cg):
                        assert z <= min(zdrop, zdrop_inv), f"{c.name} {sc}: walk skipped at score {ps} + {u}, but max_zdrop = {z} > min({zdrop}, {zdrop_inv})"
                        n_true += u == 0
                    else:
                        n_false += u == 0
                    n_units += u > 0
            assert not tap(gq, ge, q2, e2, a, 2000, 1500, w, 1, ps, n_cg, p_cg), "a z-dropped pass is never skipped"
            if w > 0:
                assert not tap(gq, ge, q2, e2, a, 1 << 30, 1 << 30, w - 1, 0, ps, n_cg, p_cg), "nor one whose band cuts the matrix"
            assert tap(gq, ge, q2, e2, a, 1 << 30, 1 << 30, -1, 0, ps, n_cg, p_cg), f"{c.name}: no band, thresholds out of reach"
    assert n_true >= 50 and n_false >= 50, (n_true, n_false)
    assert n_units >= 1000


def test_zdrop_impossible_on_the_reference_dp(product_so, oracle_lib, ref_lib):
    """What the host really hands the shortcut: the score and the trace of one global pass.  The reference's ksw_extd2_sse aligns the sequences of
    every case of up to 2 200 bases as the first pass does (KSW_EZ_APPROX_MAX, no end bonus, no z-drop inside).

    Band over the whole matrix: the score equals the path score of the pass's own trace under the dual gap costs -- the premise of the shortcut
    -- and the shortcut's own bound (bisected over the thresholds, so no threshold is left untried) is never below what the walk finds.
    Bands of 20 and 100 diagonals: where the band cuts the matrix the reference's score can exceed its trace's (by up to 558 on these cases),
    by more than the margin of the proof, and the walk then finds more than the bound computed from that score (4 705 against 4 513 on
    peak_1030_lane0_7 under (1, 9, 16, 2), band 20): those pairs must exist here, and the shortcut must refuse every pass whose band cuts the matrix."""
    import stagebind as sb
    tap = pb.zdrop_impossible_fn(C.CDLL(product_so))
    n = n_tight = n_cut = n_above = n_beyond = 0
    for sc in pc.SCORINGS:
        a, b, gq, ge = sc
        q2, e2 = pc.DUAL[sc]
        mat = sb.simple_mat(a, b, 1)
        for c in EVERY:
            if len(c.q) == 0 or len(c.t) == 0 or len(c.q) + len(c.t) > 2200:
                continue
            full = max(len(c.q), len(c.t))
            for w in (full, 100, 20):
                ez = sb.ref_extd2(ref_lib.dll, c.q, c.t, mat, gq, ge, q2, e2, w, 1 << 20, -1, 0x08)
                if ez["zdropped"] or not ez["cigar"]:                     # (the band does not reach the last cell)
                    assert w < full, c.name
                    continue
                d = pc.Case(c.name, c.family, c.t, c.q, np.ascontiguousarray(ez["cigar"], dtype=np.uint32))
                assert pc.spans(d.cigar) == (len(c.q), len(c.t)), c.name
                ps, nonmatch = path_score(d, sc)
                z = pb.oracle_zdrop_walk(oracle_lib.dll, d.q, d.t, d.cigar, sc)[0]
                bound = least_limit(tap, gq, ge, q2, e2, a, w, ez["score"], len(d.cigar), d.cigar.ctypes.data)
                if w >= full:
                    assert ez["score"] == ps, f"{c.name} {sc}: the pass scores {ez['score']}, its trace {ps}"
                    assert bound is not None and z <= bound, f"{c.name} {sc}: the walk finds {z}, the shortcut allows a skip from {bound}"
                    n += 1
                    n_tight += z == bound
                else:
                    assert bound is None, f"{c.name} {sc}: a band of {w} cuts a matrix of {full}, and the walk is skipped from {bound}"
                    n_cut += 1
                    n_above += ez["score"] > ps + a * nonmatch
                    unbanded = least_limit(tap, gq, ge, q2, e2, a, -1, ez["score"], len(d.cigar), d.cigar.ctypes.data)
                    n_beyond += unbanded is not None and z > unbanded
    assert n >= 1500 and n_tight >= 100, (n, n_tight)
    assert n_cut >= 1500 and n_above >= 50 and n_beyond >= 20, (n_cut, n_above, n_beyond)
