"""The chain sweep (pangraph_amd/csrc/pga_chain.hip) on anchor geometry chosen against it (tests/chain_cases.py), through the anchor-level tap
pga_stage_chain_anchors: f[] / p[] of EVERY anchor against the restatement's (pgo_lchain_rmq_fp, pinned to the reference by
tests/test_chain_cases_cpu.py), u / chains against the compiled reference's mg_lchain_rmq, all exact -- under the production fast kernel, under its
counting instantiation and with every segment sent to the tree kernel -- with the route counters of pga_stage_chain_routes as the proof of which
branch answered; and the tie-order-independent route (chain_all's order-event proof) on inputs chosen against it."""
import os

import numpy as np
import pytest

import chain_cases as cc
import stagebind as sb

pytestmark = pytest.mark.gpu

GROUPS = cc.groups()
WHY = ("why1_ring", "why2_cap", "why3_tie", "why4_inner")


def _check(case, got, exp, what):
    assert len(got) == len(exp)
    for qi, (g, e) in enumerate(zip(got, exp)):
        where = f"{case.name}, query {qi}, {what}"
        bad = np.flatnonzero(g["f"] != e["f"])
        assert len(bad) == 0, f"{where}: f differs at anchors {bad[:8]} (of {len(bad)}): {g['f'][bad[:8]]} vs {e['f'][bad[:8]]}"
        bad = np.flatnonzero(g["p"].astype(np.int64) != e["p"])
        assert len(bad) == 0, f"{where}: p differs at anchors {bad[:8]} (of {len(bad)}): {g['p'][bad[:8]]} vs {e['p'][bad[:8]]}"
        assert np.array_equal(g["u"], e["u"]), f"{where}: u"
        assert np.array_equal(g["chain"], e["chain"]), f"{where}: chains"


def _routes_of_group(group, gpu_lib, ref_lib, oracle_lib):
    """every case of the group under the three routes of the reference's procedure, compared anchor by anchor; -> the counters of the counting
    instantiation per case"""
    dll = gpu_lib.dll
    sb.product_chain_routes(dll)                                   # (zeroes what earlier calls left)
    routes = {}
    for case in GROUPS[group]:
        exp = sb.chain_expected(case, ref_lib.dll, oracle_lib.dll)
        _check(case, sb.product_chain_anchors(dll, case.queries, case.params, 0), exp, "production fast kernel")
        assert not any(sb.product_chain_routes(dll).values()), "the production instantiation counts nothing"
        _check(case, sb.product_chain_anchors(dll, case.queries, case.params, 1), exp, "counting fast kernel")
        routes[case.name] = sb.product_chain_routes(dll)
        print(case.name, routes[case.name])
        os.environ["PGA_CHAIN_EXACT_ONLY"] = "1"
        try:
            _check(case, sb.product_chain_anchors(dll, case.queries, case.params, 0), exp, "tree kernel only")
        finally:
            del os.environ["PGA_CHAIN_EXACT_ONLY"]
    return routes


def _sum(routes):
    return {k: sum(r[k] for r in routes.values()) for k in sb.CHAIN_ROUTES}


def _spec_of_group(group, gpu_lib, ref_lib, oracle_lib):
    """the tie-order-independent route: a query that raises no order event carries the reference's chains; one that holds neither equal candidate
    scores nor equal x raises none.  -> per case the list of (ev, need) per query"""
    out = {}
    for case in GROUPS[group]:
        exp = sb.chain_expected(case, ref_lib.dll, oracle_lib.dll)
        got = sb.product_chain_anchors(gpu_lib.dll, case.queries, case.params, 2)
        for qi, (q, g, e) in enumerate(zip(case.queries, got, exp)):
            where = f"{case.name}, query {qi}, tie-order-independent route"
            assert np.array_equal(g["f"], e["f"]) and np.array_equal(g["p"].astype(np.int64), e["p"]), f"{where}: f / p"
            if cc.free_of_order_ties(q, e["f"], case.params):
                assert g["need"] == 0, f"{where}: nothing is tied, yet the reference's order is asked for (ev {g['ev']:#x})"
            if g["need"] == 0:
                assert np.array_equal(g["u"], e["u"]) and np.array_equal(g["chain"], e["chain"]), f"{where}: no order event (ev {g['ev']:#x}), chains differ"
        out[case.name] = [(g["ev"], g["need"]) for g in got]
    return out


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_chain_routes(group, gpu_lib, ref_lib, oracle_lib):
    per_case = _routes_of_group(group, gpu_lib, ref_lib, oracle_lib)
    R = _sum(per_case)
    n_seg_flagged = sum(R[w] for w in WHY)
    if group == "colinear":
        assert R["stretch"] > 0 and n_seg_flagged == 0, R
        for name in ("colinear_step10", "colinear_alternating", "colinear_broken"):
            assert per_case[name]["stretch"] > 0, (name, per_case[name])
        r = per_case["colinear_step30"]                            # dd == 0 but dg > span: never "exact", so no stretch -- the single shortcut
        assert r["stretch"] == 0 and r["single"] > 0, r
    elif group == "shortcut_edges":
        assert n_seg_flagged == 0, R
        assert per_case["bound_last_anchor"]["inner_reg"] > 0 and per_case["inner_y_edge"]["inner_reg"] > 0 and per_case["y_range_edge"]["stretch"] > 0, per_case
    elif group == "wrap":
        assert n_seg_flagged == 0, R
        for name, r in per_case.items():                             # 20 rows: the chunked form, 6 rows: the register form
            assert r["inner_chunk" if "x20" in name else "inner_reg"] > 0 and ("x20" in name or r["inner_chunk"] == 0), (name, r)
    elif group == "overflow_s4":
        assert R["why1_ring"] > 0, R
    elif group == "overflow_s6":
        assert n_seg_flagged == 0 and R["fast"] > 0, R
    elif group == "cap":
        assert R["why2_cap"] > 0 and R["stretch"] == 0 and R["single"] == 0, R
        for name, r in per_case.items():
            if name.startswith("cap"):
                assert r["why2_cap"] > 0, (name, r)
    elif group == "tie":
        for name, r in per_case.items():
            assert r["why3_tie"] > 0, (name, r)
    elif group == "grid12":
        assert R["inner_reg"] > 0 and R["rerank"] > 0 and R["inner_chunk"] == 0 and n_seg_flagged == 0, R
    elif group == "grid20":
        assert R["inner_chunk"] > 0 and R["rerank"] > 0 and n_seg_flagged == 0, R
    elif group == "grid34":
        for name, r in per_case.items():
            assert r["why4_inner"] > 0, (name, r)
    elif group == "summary":
        r = per_case["scatter"]
        assert r["summary"] > 0 and r["summary_scan"] > 0, r
    elif group == "interleave_70":
        assert R["bt_reload"] > 0, R
    if group.startswith("grid"):
        for name, r in per_case.items():
            if name.endswith("_skip0") or name.endswith("_skip2"):
                assert r["skip_stop"] > 0, (name, r)


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_tie_order_independent_route(group, gpu_lib, ref_lib, oracle_lib):
    per_case = _spec_of_group(group, gpu_lib, ref_lib, oracle_lib)
    if group == "equal_targets":       # candidates of equal score, chains that start at distinct target positions: the emission order cannot show
        for ev, need in per_case["equal_targets"]:
            assert ev & 8 and not ev & 4 and need == 0, (ev, need)
    elif group == "equal_starts":      # ... that start at ONE target position: equal keys in compact_a's sort, in the candidate sort's tie order
        for ev, need in per_case["equal_starts"]:
            assert ev & 4 and ev & 8 and ev & 16 and need == 1, (ev, need)
    elif group == "equal_fork":        # two chains of equal score over a shared trunk: whichever is walked second stops at (or is marked by) the other
        for ev, need in per_case["equal_fork"]:
            assert ev & 3 and need == 1, (ev, need)
