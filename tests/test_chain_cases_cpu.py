"""The anchor-level chain cases (tests/chain_cases.py) on the CPU: every case through the compiled reference's mg_lchain_rmq and through the
restatement (oracle/pgo_chain.c), which must agree on u and the chains; pgo_lchain_rmq_fp, whose f[] / p[] the GPU tests compare against, must
return what pgo_lchain_rmq returns.  The properties the GPU assertions of tests/test_gpu_chain_routes.py rely on are pinned here, so that a case
that no longer reaches its edge fails here and not silently there."""
import numpy as np
import pytest

import chain_cases as cc
import stagebind as sb

CASES = cc.all_cases()
M32 = np.uint64(0xffffffff)


def _xy(q):
    """target position within (strand, target), query position, the (strand, target) word"""
    return (q[:, 0] & M32).astype(np.int64), (q[:, 1] & M32).astype(np.int64), q[:, 0] >> np.uint64(32)


def _window(q, dist):
    """the most anchors below an anchor and within dist of it in x, same strand and target: what the trees of lchain.c:295-303 hold at most"""
    x, _, tg = _xy(q)
    best = 0
    for t in np.unique(tg):
        xs = x[tg == t]
        best = max(best, int((np.arange(len(xs)) - np.searchsorted(xs, xs - dist, side="left")).max()))
    return best


def test_generators_are_deterministic_and_sorted():
    again = {c.name: c for c in cc.all_cases()}
    for c in CASES:
        assert sum(len(q) for q in c.queries) <= 20_000, c.name
        for q, q2 in zip(c.queries, again[c.name].queries):
            assert q.dtype == np.uint64 and q.shape == (len(q), 2) and np.array_equal(q, q2), c.name
            if len(q) > 1:
                dx = q[1:, 0].astype(object) - q[:-1, 0].astype(object)
                assert all(d >= 0 for d in dx), f"{c.name}: anchors ascend in x"
                assert len(np.unique(q, axis=0)) == len(q), f"{c.name}: no anchor twice"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_reference_vs_restatement(case, ref_lib, oracle_lib):
    exp = sb.chain_expected(case, ref_lib.dll, oracle_lib.dll)
    n_chains = []
    for qi, (q, e) in enumerate(zip(case.queries, exp)):
        assert np.array_equal(e["u"], e["o_u"]) and np.array_equal(e["chain"], e["o_chain"]), f"{case.name}: query {qi}, restatement vs reference"
        u2, ch2 = sb.oracle_chain_np(oracle_lib.dll, q, case.params)
        assert np.array_equal(u2, e["o_u"]) and np.array_equal(ch2, e["o_chain"]), f"{case.name}: query {qi}, pgo_lchain_rmq_fp vs pgo_lchain_rmq"
        assert len(e["f"]) == len(q) and np.all(e["p"] < np.arange(len(q))) and np.all(e["p"] >= -1)
        n_chains.append(len(e["u"]))
    if case.chains:
        assert sum(n_chains) > 0, f"{case.name} is meant to chain"
    pins = case.pins
    if "n_chains" in pins:
        assert n_chains == pins["n_chains"], case.name
    if "n_anchors" in pins:
        assert sum(len(q) for q in case.queries) == pins["n_anchors"]
    mg = max(case.params.max_gap, case.params.bw)
    if "window_min" in pins:
        assert max(_window(q, mg) for q in case.queries) >= pins["window_min"], case.name
    if "window_max" in pins:
        assert max(_window(q, mg) for q in case.queries) <= pins["window_max"], case.name
    if "inner_min" in pins:
        w = max(_window(q, case.params.rmq_inner_dist) for q in case.queries)
        assert w >= pins["inner_min"] and (pins["inner_max"] is None or w <= pins["inner_max"]), (case.name, w)
    if pins.get("no_tie"):
        assert sum(sb.oracle_tie_count(oracle_lib.dll, q, case.params) for q in case.queries) == 0, f"{case.name}: a tied minimum would pre-empt the inner scan"
    if pins.get("tie"):
        assert sum(sb.oracle_tie_count(oracle_lib.dll, q, case.params) for q in case.queries) > 0, case.name
        found = False
        for q, e in zip(case.queries, exp):                       # two anchors of equal f and equal x + y inside one range-min query
            x, y, _ = _xy(q)
            for i in range(len(q)):
                inside = (x < x[i]) & (x[i] - x <= mg) & (y < y[i]) & (y > y[i] - mg)
                keys = list(zip(e["f"][inside].tolist(), (x + y)[inside].tolist()))
                found |= len(set(keys)) < len(keys)
        assert found, case.name
    if "last_p" in pins:
        assert exp[0]["p"][-1] == pins["last_p"] and exp[0]["f"][-1] == pins["last_f"], (exp[0]["p"][-3:], exp[0]["f"][-3:])
    if "last_ps" in pins:
        assert [int(e["p"][-1]) for e in exp] == pins["last_ps"], [e["p"][-2:] for e in exp]
    for (qi, at), v in pins.get("p_at", {}).items():
        assert exp[qi]["p"][at] == v, (qi, at, exp[qi]["p"][at])
    for (qi, at), v in pins.get("f_at", {}).items():
        assert exp[qi]["f"][at] == v, (qi, at, exp[qi]["f"][at])
    if "n_min" in pins:
        assert min(len(q) for q in case.queries) >= pins["n_min"]
    if "n_first_block" in pins:
        q, e = case.queries[0], exp[0]
        x, y, _ = _xy(q)
        assert len(q) > 64 and e["f"][62] == e["f"][63] and x[62] + y[62] == x[63] + y[63] and np.all(e["f"][:62] + 0.076 * (x + y)[:62] < e["f"][63] + 0.076 * (x + y)[63])
    if "equal_x_runs" in pins:
        x = case.queries[0][:, 0]
        for s in pins["equal_x_runs"]:
            assert x[s] == x[s + 1], s
        assert x[0] == x[2] and x[62] == x[66] and x[126] == x[130] and x[61] != x[62] and x[66] != x[67]
    if pins.get("index0"):
        # the anchor that shares y with anchor 0: unchained where that is the query's anchor 0, chained to the anchor in between behind the segment cut
        (q0, q1), (e0, e1) = case.queries, exp
        assert e0["p"][2] == -1 and e1["p"][2] == -1 and e0["f"][2] == cc.SPAN
        assert q0[11, 1] == q0[13, 1] and e0["p"][13] == 12 and e0["f"][13] == 20


def test_some_cases_are_free_of_order_ties(ref_lib, oracle_lib):
    """the tie-order-independent route must not ask for the reference's order where no two candidates score alike and no two anchors share x: the
    GPU test derives that from f[] per query, and this keeps the derivation from being vacuous"""
    free = 0
    for case in CASES:
        for q, e in zip(case.queries, sb.chain_expected(case, ref_lib.dll, oracle_lib.dll)):
            free += cc.free_of_order_ties(q, e["f"], case.params) and len(e["u"]) > 0
    assert free > 50
