"""pga_plan_merge (pga_reweave.hip: reweave's intervals and promises on the device) and pangraph_amd.reweave against the restatement
tests/reweave_ref.py and the reference's own unit-test values (tests/golden/reweave_vectors.json).  Every comparison is exact: every field
of every list, offsets and counters included."""
import ctypes as C
import json
import os

import pytest

import reweave_gen as rg
import reweave_ref as rr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import reweave as rw  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
cg = rr.parse_cigar


def _resident(groups):
    return batch.ResidentBatch(batch.PreparedBatch([[b["consensus"] for b in g] for g in groups if g]))


def check_level(dll, groups, matches, thr, resident=False):
    """the product against the restatement, field by field"""
    rb = _resident(groups) if resident else None
    try:
        got = rw.plan_merge(groups, matches, thr, batch=rb, dll=dll)
    finally:
        if rb is not None:
            rb.close()
    exp = rr.expected_call(groups, matches, thr, resident=resident)
    assert got["counters"] == exp["counters"] and got["n_failed"] == exp["n_failed"]
    for name in ("matches", "blocks", "intervals", "slice_intervals", "cigars", "promises"):
        g, e = got[name], exp[name]
        assert (g is None) == (e is None), name
        if e is not None:
            assert len(g) == len(e), name
            for k, (a, b) in enumerate(zip(g, e)):
                assert a == b, (name, k, a, b)
    return got


# ---------------------------------------------------------------- 1. the reference's own values
def test_reference_vectors(gpu_lib):
    dll = gpu_lib.dll
    # test_reweave: ids, anchors, intervals, promise order, orientations and CIGARs
    v = VEC["reweave"]
    order = sorted(int(b) for b in v["blocks"])
    blks = [{"block_id": b, "consensus": "ACGT" * (v["blocks"][str(b)][0] // 4) + "A" * (v["blocks"][str(b)][0] % 4), "depth": v["blocks"][str(b)][1]} for b in order]
    matches = [{"group": 0, "qry": order.index(a["qry"]["name"]), "ref": order.index(a["reff"]["name"]), "qry_start": a["qry"]["start"], "qry_end": a["qry"]["end"],
                "ref_start": a["reff"]["start"], "ref_end": a["reff"]["end"], "reverse": a["reverse"], "cigar": cg(a["cigar"])} for a in v["alignments"]]
    for resident in (False, True):
        got = check_level(dll, [blks], matches, v["thr_len"], resident)
        by_match = {p["match"]: p for p in got["promises"]}
        for e in v["expected_promises"]:
            p = by_match[e["match"]]
            a, q = got["intervals"][p["anchor_interval"]], got["intervals"][p["append_interval"]]
            assert [order[p["anchor_block"]], a["start"], a["end"]] == e["anchor"] and [order[p["append_block"]], q["start"], q["end"]] == e["append"]
            assert p["reverse"] == int(e["reverse"]) and p["cigar"] == cg(e["cigar"])
        assert [p["new_block_id"] for p in got["promises"]] == sorted(m["new_block_id"] for m in got["matches"])
        for b in got["blocks"]:
            gaps = [[i["start"], i["end"]] for i in got["intervals"][b["first_interval"]:b["first_interval"] + b["n_intervals"]] if not i["aligned"]]
            assert gaps == v["expected_unaligned"].get(str(order[b["block"]]), [])
    # pangraph_interval.rs: create_intervals / refine_intervals on the example (the four hits paired with blocks of their own)
    v = VEC["intervals"]
    blks = [{"block_id": v["block_id"], "consensus": "ACGT" * (v["block_length"] // 4), "depth": 9}]
    matches = []
    for k, h in enumerate(v["hits"]):
        ln = h["end"] - h["start"]
        blks.append({"block_id": 100 + k, "consensus": "T" * ln, "depth": 1})
        matches.append({"group": 0, "ref": 0, "qry": k + 1, "ref_start": h["start"], "ref_end": h["end"], "qry_start": 0, "qry_end": ln, "reverse": h["reverse"], "cigar": [("M", ln)]})
    got = check_level(dll, [blks], matches, v["thr_len"])
    mine = got["intervals"][got["blocks"][0]["first_interval"]:][:got["blocks"][0]["n_intervals"]]
    assert got["blocks"][0]["block"] == 0
    assert [(i["start"], i["end"], i["extend_left"], i["extend_right"], bool(i["aligned"])) for i in mine] == \
        [(x["start"], x["end"], x["extend_left"] or 0, x["extend_right"] or 0, x["new_block_id"] is not None) for x in v["refined"]]
    assert [i["new_block_id"] for i in mine if not i["aligned"]] == [rr.gap_id(v["block_id"], x["start"], x["end"]) for x in v["refined"] if x["new_block_id"] is None]
    got = check_level(dll, [blks], matches, 0)
    assert [(i["start"], i["end"]) for i in got["intervals"][got["blocks"][0]["first_interval"]:][:got["blocks"][0]["n_intervals"]]] == [(s, e) for s, e, _ in v["created"]]
    # test_split_block: a qry-side anchor's CIGAR is switched; the reverse one is the append side
    v = VEC["split_block"]
    blks = [{"block_id": 1, "consensus": "A" * 130, "depth": 3}, {"block_id": 2, "consensus": "C" * 150, "depth": 1}, {"block_id": 3, "consensus": "G" * 1050, "depth": 4}]
    a0, a1 = v["alignments"]
    matches = [{"group": 0, "qry": 0, "ref": 1, "qry_start": 10, "qry_end": 50, "ref_start": 100, "ref_end": 150, "reverse": False, "cigar": cg(a0["cigar"])},
               {"group": 0, "qry": 2, "ref": 0, "qry_start": 1000, "qry_end": 1050, "ref_start": 80, "ref_end": 130, "reverse": True, "cigar": cg(a1["cigar"])}]
    got = check_level(dll, [blks], matches, v["thr_len"])
    b = got["blocks"][0]
    assert [[i["start"], i["end"], bool(i["aligned"])] for i in got["intervals"][b["first_interval"]:b["first_interval"] + b["n_intervals"]]] == v["expected_intervals"]
    assert [m["anchor"] for m in got["matches"]] == [1, 1]
    p0 = [p for p in got["promises"] if p["match"] == 0][0]
    assert p0["cigar"] == cg("10D10I10M10D40M")                                      # the switched CIGAR of the vector behind the 10-letter overhang of block 1


def test_update_cigar_known_answers(gpu_lib):
    """reweave.rs:1139-1204 through the product: the base CIGAR on a ref-side anchor, the extensions as short gaps of that size"""
    for base, anchor, append, reverse, expected in rg.UPDATE_CIGAR_CASES:
        al, ar, pl, pr_ = anchor[0] or 0, anchor[1] or 0, append[0] or 0, append[1] or 0
        L = rg.Level(1)
        L.group([[("g", al), ("h", 40, 0), ("g", ar)], [("g", pl), ("h", 40, 0), ("g", pr_)]], pairs={0: {"cigar": cg(base), "reverse": reverse}}, depths=[2, 1])
        got = check_level(gpu_lib.dll, *L.level(), 20)
        assert got["matches"][0]["anchor"] == 0 and got["promises"][0]["cigar"] == cg(expected)


def test_anchor_cases(gpu_lib):
    """the eleven rstest cases of assign_anchor_block, with and without a batch"""
    groups, matches = rg.anchor_cases_level()
    for resident in (False, True):
        got = check_level(gpu_lib.dll, groups, matches, 1, resident)
        assert [("ref", "qry")[m["anchor"]] for m in got["matches"]] == [c[3] for c in rg.ANCHOR_CASES]
        assert [m["route"] == 0 for m in got["matches"]] == [c[0][1] != c[1][1] for c in rg.ANCHOR_CASES]


# ---------------------------------------------------------------- 2. hits and intervals
def test_hit_counts_groups_and_scans(gpu_lib):
    groups, matches = rg.hits_level()
    got = check_level(gpu_lib.dll, groups, matches, rg.THR)
    assert got["counters"]["hits"] == 2 * len(matches) > 512 and got["counters"]["intervals_after"] > 256


@pytest.mark.parametrize("k", (0, 1, 2))
def test_promise_counts_around_a_wave(gpu_lib, k):
    groups, matches = rg.promise_levels()[k]
    assert len(check_level(gpu_lib.dll, groups, matches, rg.THR)["promises"]) == (63, 64, 65)[k]


# ---------------------------------------------------------------- 3. refinement
def test_refinement_rules(gpu_lib):
    groups, matches = rg.refine_level()
    got = check_level(gpu_lib.dll, groups, matches, rg.THR)
    assert got["counters"]["intervals_before"] > got["counters"]["intervals_after"]
    got = check_level(gpu_lib.dll, groups, matches, 0)                              # thr_len = 0: nothing is short
    assert got["counters"]["intervals_before"] == got["counters"]["intervals_after"]
    check_level(gpu_lib.dll, groups, matches, 1)


@pytest.mark.parametrize("name", sorted(rg.failing_blocks()))
def test_failing_block_nulls_the_lists(gpu_lib, name):
    good = rg.refine_level()
    L = rg.Level(5)
    L.groups, L.matches = [list(g) for g in good[0]], list(good[1])                # a group that succeeds in front: a failure anywhere nulls the lists
    L.group(rg.failing_blocks()[name])
    got = check_level(gpu_lib.dll, *L.level(), rg.THR)
    assert got["n_failed"] == 1 and got["intervals"] is None and got["promises"] is None
    assert [b["status"] for b in got["blocks"] if b["status"]] == [5 if name in ("gap_before_short_hit", "gap_between") else 1]


# ---------------------------------------------------------------- 4. CIGARs
def test_cigars(gpu_lib):
    groups, matches = rg.cigar_level()
    got = check_level(gpu_lib.dll, groups, matches, rg.THR)
    assert got["counters"]["cigar_out"] > got["counters"]["cigar_in"] > 6000


# ---------------------------------------------------------------- 5. the anchor decision
def test_anchor_routes_with_and_without_a_batch(gpu_lib):
    groups, matches = rg.anchor_level()
    a = check_level(gpu_lib.dll, groups, matches, rg.THR, resident=False)
    b = check_level(gpu_lib.dll, groups, matches, rg.THR, resident=True)
    strip = lambda r: [(m["new_block_id"], m["anchor"], m["ref_n"], m["qry_n"]) for m in r["matches"]]
    assert strip(a) == strip(b) and a["intervals"] == b["intervals"] and a["promises"] == b["promises"] and a["cigars"] == b["cigars"]
    ca, cb = a["counters"], b["counters"]
    assert ca["by_mask"] == 0 and ca["by_letters"] == len(matches) - 2 and ca["by_depth"] == 2
    assert cb["by_mask"] > 5 and cb["by_letters"] > 5 and cb["by_mask"] + cb["by_letters"] == len(matches) - 2 and cb["by_depth"] == 2
    assert {m["route"] for m in a["matches"]} == {0, 2} and {m["route"] for m in b["matches"]} == {0, 1, 2}


@pytest.mark.parametrize("seed", range(6))
def test_random_levels(gpu_lib, seed):
    groups, matches = rg.random_level(seed, fail=seed % 3 == 2)
    check_level(gpu_lib.dll, groups, matches, rg.THR, resident=seed % 2 == 1)


# ---------------------------------------------------------------- 6. malformed input
def test_malformed_input_fails_the_call(gpu_lib):
    dll = gpu_lib.dll
    L = rg.Level(7)
    L.group([[("g", 5), ("h", 30, 0), ("h", 25, 1)], [("h", 30, 0)], [("h", 25, 1)]])
    groups, matches = L.level()
    check_level(dll, groups, matches, 3)

    def bad(match, groups=groups, matches=matches, thr=3, **kw):
        with pytest.raises(batch.PgaError, match=match):
            rw.plan_merge(groups, matches, thr, dll=dll, **kw)

    edit = lambda k, **kw: [dict(m, **kw) if i == k else m for i, m in enumerate(matches)]
    bad("itself", matches=edit(0, qry=matches[0]["ref"]))
    bad("outside its group", matches=edit(0, qry=3))
    bad("outside its group", matches=edit(1, ref=-1))
    bad("group outside", matches=edit(1, group=1))
    bad("empty hit", matches=edit(0, qry_end=matches[0]["qry_start"]))
    bad("outside its block", matches=edit(0, ref_end=10 ** 6))
    bad("overlap", matches=edit(1, **{s + "_start": matches[1][s + "_start"] - 1 for s in ("ref", "qry") if matches[1][s] == 0}))
    bad("overlap|same new block id", matches=matches + [matches[0]], thr=0)          # (one id twice means the same two hits twice: either check may speak first)
    bad("Unexpected CIGAR operation", matches=edit(0, cigar=[("M", 5), ("S", 2)]))
    bad("Unexpected CIGAR operation", matches=edit(1, cigar=[("N", 5)]))
    bad("2\\^28", groups=[[dict(b) for b in g] for g in groups], matches=edit(0, cigar=[("D", (1 << 28) - 3), ("M", 5)]), thr=6)
    bad("CIGAR outside the pool", matches=edit(1, n_cigar=10 ** 6))
    bad("null letters", groups=[[dict(groups[0][0], consensus=None, cons_len=60)] + groups[0][1:]])
    bad("share the block id", groups=[[dict(groups[0][0], block_id=groups[0][1]["block_id"])] + groups[0][1:]])
    rb = _resident(groups)
    try:
        bad("seq_index outside", batch=rb, seq_index=[0, 1, 3])
        bad("differs from its sequence", batch=rb, seq_index=[1, 0, 2])
    finally:
        rb.close()
    # n_matches == 0: empty lists
    got = rw.plan_merge(groups, [], 3, dll=dll)
    assert got["matches"] == [] and got["blocks"] == [] and got["intervals"] == [] and got["promises"] == [] and got["n_failed"] == 0
    check_level(dll, groups, matches, 3)                                             # the library is as before


# ---------------------------------------------------------------- 7. the chain
def test_chain_plan_slice_solve(gpu_lib, oracle_lib):
    """pga_plan_merge -> pga_slice_blocks -> pga_solve_promises on a small synthetic merge (a forward and a reverse match, each with short
    overhangs on both blocks), pointer arithmetic only between the calls, against reweave_ref + slice_ref + promise_ref."""
    import numpy as np
    import mapvarbind as mb
    import promise_ref as pr
    import slice_ref as sr
    from pangraph_amd import slice as sl
    from pangraph_amd.mapvar import del_t, ins_t, params, res_t, sub_t
    from pangraph_amd.reconsensus import rc_member_t
    dll = gpu_lib.dll
    rng = np.random.default_rng(12)
    thr = 20
    E = lambda g, shift: {"subs": [(p + shift, a) for p, a in g["subs"]], "dels": [(p + shift, n) for p, n in g["dels"]], "inss": [(p + shift, s) for p, s in g["inss"]]}
    groups, matches, members, nodes = [], [], [], []                          # members / nodes: per block, flat
    for g, reverse in enumerate((False, True)):
        anchor = mb.random_seq(rng, 300)
        oriented = mb.mutate(rng, anchor, snp=0.03, indel=0.01, max_indel=6)
        append = pr.reverse_complement(oriented) if reverse else oriented
        a = mb.oracle_map_variations(oracle_lib.dll, anchor, oriented, 0, 60, want_aln=True)
        assert a["status"] == 0
        cigar = [(op, n) for n, op in pr.cigar_from_alignment(a["ref_aln"], a["qry_aln"])]
        mem_b = []
        for _ in range(3):                                                    # the append block's members, spelled against its consensus
            seq = mb.mutate(rng, append, snp=0.02, indel=0.005, max_indel=4)
            v = mb.oracle_map_variations(oracle_lib.dll, append, seq, 0, 40)
            assert v["status"] == 0
            mem_b.append(E(v, 3))
        cons_a = mb.random_seq(rng, 5) + anchor + mb.random_seq(rng, 30)      # [5 short][hit][30 stays]
        cons_b = mb.random_seq(rng, 3) + append + mb.random_seq(rng, 2)       # [3 short][hit][2 short]
        groups.append([{"block_id": 10 + g, "consensus": cons_a, "depth": 4}, {"block_id": 20 + g, "consensus": cons_b, "depth": 3}])
        matches.append({"group": g, "ref": 0, "qry": 1, "ref_start": 5, "ref_end": 305, "qry_start": 3, "qry_end": 3 + len(append), "reverse": reverse, "cigar": cigar})
        members += [[{"subs": [(7, "A" if cons_a[7] != "A" else "C")], "dels": [(100, 4)], "inss": []}] * 1, mem_b]
        nodes += [[(1000, 1000 + len(cons_a) - 4, 10 ** 6, False, False)], [(50 * k, 50 * k + len(mb.apply_edit(cons_b, e)), 10 ** 6, k == 1, False) for k, e in enumerate(mem_b)]]
    exp = rr.expected_call(groups, matches, thr)
    K = rw._Packed(groups, matches)
    plan = rw.plan_merge_raw(K.args(), thr, dll=dll, keep=K)
    free_slice = None
    try:
        assert plan.to_lists()["promises"] == exp["promises"] and plan.to_lists()["slice_intervals"] == exp["slice_intervals"]
        o = plan.out
        flat = [b for g in groups for b in g]
        order = [o.blocks[k].block for k in range(o.n_blocks)]
        S = sl._Packed([dict(consensus=flat[b]["consensus"], members=members[b], nodes=nodes[b], intervals=[(0, 0, 0)] * o.blocks[k].n_intervals) for k, b in enumerate(order)])
        sl._bind(dll)
        sout = sl.slice_out_t()
        sargs = list(S.args())
        sargs[2] = C.cast(o.slice_intervals, C.c_void_p)                       # the plan's own table, not a copy
        assert dll.pga_slice_blocks(*sargs, C.byref(sout)) == 0, dll.pga_last_error()
        free_slice = lambda: dll.pga_slice_free(C.byref(sout))
        P = rw.promise_args(plan, K.B)
        dll.pga_solve_promises.restype = C.c_int
        dll.pga_solve_promises.argtypes = [C.c_int64] + [C.c_void_p] * 8 + [C.POINTER(C.POINTER(sub_t)), C.POINTER(C.POINTER(del_t)), C.POINTER(C.POINTER(ins_t)), C.POINTER(C.POINTER(C.c_char))]
        dll.pga_free.argtypes = [C.c_void_p]
        n_checked = 0
        for p in range(o.n_promises):
            r, e = o.promises[p], exp["promises"][p]
            res = sout.slices[r.append_interval]                               # slices are numbered as the plan's intervals are
            ai, qi = exp["intervals"][e["anchor_interval"]], exp["intervals"][e["append_interval"]]
            cons_anchor, cons_append = flat[e["anchor_block"]]["consensus"], flat[e["append_block"]]["consensus"]
            iv = sr.interval(qi["start"], qi["end"], True, False, bool(qi["reverse"]))
            _, kept, dropped = sr.block_slice(cons_append, members[e["append_block"]], nodes[e["append_block"]], iv)
            assert res.n_kept == len(kept) == 3 and not dropped
            want = pr.solve_promise(oracle_lib.dll, (cons_anchor[ai["start"]:ai["end"]], cons_append[qi["start"]:qi["end"]], bool(e["reverse"]), [(n, op) for op, n in e["cigar"]],
                                                     [{k: m[k] for k in ("subs", "dels", "inss")} for m in kept]))
            first = sout.members[res.member_off]
            P[p].n_members = res.n_kept
            R = (res_t * res.n_kept)()
            subs = C.POINTER(sub_t)(); dels = C.POINTER(del_t)(); inss = C.POINTER(ins_t)(); iseq = C.POINTER(C.c_char)()
            at = lambda ptr, k, t: (C.addressof(ptr.contents) + k * C.sizeof(t)) if ptr else None
            rc = dll.pga_solve_promises(1, C.byref(P[p]), at(sout.counts, res.member_off, rc_member_t), at(sout.subs, first.sub_off, sub_t), at(sout.dels, first.del_off, del_t),
                                        at(sout.inss, first.ins_off, ins_t), S.L, C.byref(params()), R, C.byref(subs), C.byref(dels), C.byref(inss), C.byref(iseq))
            assert rc == 0, dll.pga_last_error()
            try:
                base = C.addressof(iseq.contents) if iseq else 0
                for t, w in enumerate(want):
                    x = R[t]
                    got = dict(status=x.status, score=x.score, attempts=x.attempts, hit_boundary=x.hit_boundary,
                               subs=[(subs[x.sub_off + k].pos, chr(subs[x.sub_off + k].alt)) for k in range(x.n_subs)],
                               dels=[(dels[x.del_off + k].pos, dels[x.del_off + k].len) for k in range(x.n_dels)],
                               inss=[(inss[x.ins_off + k].pos, C.string_at(base + inss[x.ins_off + k].seq_off, inss[x.ins_off + k].len).decode()) for k in range(x.n_inss)])
                    assert got == w, (p, t, got, w)
                    n_checked += got["status"] == 0
            finally:
                for ptr in (subs, dels, inss, iseq):
                    if ptr:
                        dll.pga_free(C.cast(ptr, C.c_void_p))
        assert n_checked >= 4 and {e["reverse"] for e in exp["promises"]} == {0, 1}
        assert sorted(p["n_cigar"] - len(matches[p["match"]]["cigar"]) for p in exp["promises"]) != [0, 0]      # the overhangs reached the CIGARs
    finally:
        if free_slice:
            free_slice()
        plan.free()


def test_graph_level_on_the_device(gpu_lib):
    """pangraph_amd.reweave.reweave with the two device calls against the same function over the restatements (which the CPU suite holds
    against test_reweave's positions, strands and block identities)"""
    import slice_ref as sr
    g0, matches = rg.reference_graph(VEC)
    g1, _ = rg.reference_graph(VEC)
    thr = VEC["reweave"]["thr_len"]
    slicer = lambda bl: sr.slice_blocks([dict(b, intervals=[sr.interval(s, e, bool(f), False, bool(f)) for s, e, f in b["intervals"]]) for b in bl])
    want_g, want_p = rw.reweave(g0, matches, thr, plan=rr.expected_call, slicer=slicer)
    got_g, got_p = rw.reweave(g1, matches, thr, dll=gpu_lib.dll)
    assert got_g == want_g and got_p == want_p and len(got_p) == 4
    # thr_len 150: block 20's gap [200, 300) is short and so is the hit behind it -- code 5 at interval 1, the first failing block in order
    with pytest.raises(rw.ReweaveError) as want:
        rw.reweave(rg.reference_graph(VEC)[0], matches, 150, plan=rr.expected_call, slicer=slicer)
    assert str(want.value) == "block 20: refine_intervals fails with code 5 at interval 1"
    with pytest.raises(rw.ReweaveError) as got:
        rw.reweave(rg.reference_graph(VEC)[0], matches, 150, dll=gpu_lib.dll)
    assert str(got.value) == str(want.value)
