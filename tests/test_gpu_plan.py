"""The device region planner (pangraph_amd/csrc/pga_plan.hip: k_plan_regions, k_plan_cut, k_plan_probe, k_plan_collapse and the host sequence
plan_regions) through its tap pga_stage_plan, compared exactly with the reference's own code (tests/planbind.py: expected) on the cases of
tests/plan_cases.py, whose pins tests/test_plan_cases_cpu.py asserts on the reference alone.  Every field of PlanOut, every PlanItem in item
order, every anchor word after the call and every status; nothing is sampled and there is no tolerance.
"""
import numpy as np
import pytest

import plan_cases as pcs
import planbind as pb

pytestmark = pytest.mark.gpu

CASE_FAMILIES = [f for f in pcs.FAMILIES if f != "random"]


@pytest.fixture(scope="module", autouse=True)
def _shim():
    pb.ref_plan_dll()                                                           # skips only where oracle/_ref/ was not built


def differences(G, R):
    """what the device's answer R for group G differs in from the reference's, as a list of strings (empty: identical)"""
    E = pb.expected(G)
    bad = []
    for r in range(len(G.regions)):
        got, want = R["out"][r], E["out"][r]
        st = int(want[0])
        # a region over the cap goes back to the host route untouched: status and the as1-independent fields (the extent) are compared
        fields = pb.OUT_FIELDS[:9] if st == 2 else pb.OUT_FIELDS
        d = {f: (int(got[k]), int(want[k])) for k, f in enumerate(pb.OUT_FIELDS) if f in fields and got[k] != want[k]}
        if d:
            bad.append(f"region {r} {G.regions[r]} (device, reference): {d}")
        gi, wi = R["items"][r][:, :9], E["items"][r]
        if gi.shape != wi.shape or not np.array_equal(gi, wi):
            k = next((k for k in range(min(len(gi), len(wi))) if not np.array_equal(gi[k], wi[k])), min(len(gi), len(wi)))
            bad.append(f"region {r}: {len(gi)} items, reference {len(wi)}; first difference at item {k}: "
                       f"{dict(zip(pb.ITEM_FIELDS, gi[k].tolist())) if k < len(gi) else None} against {dict(zip(pb.ITEM_FIELDS, wi[k].tolist())) if k < len(wi) else None}")
    for j, (got, want) in enumerate(zip(R["anchors"], E["anchors"])):
        if not np.array_equal(got, want):
            i = int(np.nonzero((got != want).any(axis=1))[0][0])
            bad.append(f"query {j}: {int((got != want).any(axis=1).sum())} anchor words differ, the first at anchor {i}: {int(got[i, 0]):#x} {int(got[i, 1]):#x} "
                       f"against {int(want[i, 0]):#x} {int(want[i, 1]):#x}")
    return bad


def check_groups(dll, groups):
    bad = []
    for G in groups:
        d = differences(G, pb.product_plan(dll, G))
        if d:
            bad.append(f"{G.name}: " + "; ".join(d[:4]))
    assert not bad, f"{len(bad)} of {len(groups)} cases differ from the reference:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("fam", CASE_FAMILIES)
def test_family(fam, gpu_lib):
    check_groups(gpu_lib.dll, pcs.family(fam))


@pytest.mark.parametrize("part", range(4))
def test_random_groups(part, gpu_lib):
    groups = pcs.family("random")[part::4]
    check_groups(gpu_lib.dll, groups)
    for G in groups:                                                             # none may be left out
        assert (pb.expected(G)["out"][:, 0] == 0).all()


def test_host_routes_taken(gpu_lib):
    """the host cases are what they claim: more than 1024 regions (device copies), and at most 1024 regions with more than 8192 items (records
    through pinned memory, items through a device copy); a status-2 and a status-3 region own no items, the regions around them do"""
    by = {g.name: g for g in pcs.family("host")}
    assert len(by["host_1025_regions"].regions) == 1025
    G = by["host_1024_regions_9216_items"]
    R = pb.product_plan(gpu_lib.dll, G)
    assert len(G.regions) == 1024 and sum(len(x) for x in R["items"]) == 9216
    R = pb.product_plan(gpu_lib.dll, by["host_status_mix"])
    assert R["out"][:, 0].tolist() == [0, 3, 2, 0] and [len(x) > 0 for x in R["items"]] == [True, False, False, True]
    R = pb.product_plan(gpu_lib.dll, by["host_empty_list"])
    assert R["out"].shape[0] == 0 and R["items"] == [] and np.array_equal(R["anchors"][0], by["host_empty_list"].queries[0][1])


def test_all_regions_in_one_call(gpu_lib):
    """the random groups' regions keep their answers when a call holds them in another order (regions of one call are independent)"""
    for G in pcs.family("random")[:6]:
        order = list(range(len(G.regions)))[::-1]
        R = pb.product_plan(gpu_lib.dll, G, regions=[G.regions[r] for r in order])
        E = pb.expected(G)
        for k, r in enumerate(order):
            assert np.array_equal(R["out"][k], E["out"][r]) and np.array_equal(R["items"][k][:, :9], E["items"][r]), f"{G.name}: region {r}"
        assert all(np.array_equal(a, b) for a, b in zip(R["anchors"], E["anchors"]))


# ---------------------------------------------------------------- refusals: by message, and nothing reaches a kernel
def _base_group():
    return next(g for g in pcs.family("cut") if g.name == "cut_cnt66")


def _refused(dll, G, message, **kw):
    with pytest.raises(RuntimeError) as e:
        pb.product_plan(dll, G, **kw)
    assert message in str(e.value), str(e.value)
    # the call's buffers came back as they went in: no record written, no anchor flagged
    assert not e.value.out.any()
    assert all(np.array_equal(a, b) for a, b in zip(e.value.anchors, [a for _, a in kw.get("queries", G.queries)]))


def _with_anchor(G, i, x=None, y=None):
    q, a = G.queries[0]
    a = a.copy()
    if x is not None:
        a[i, 0] = x
    if y is not None:
        a[i, 1] = y
    return [(q, a)]


def test_refusals(gpu_lib):
    dll = gpu_lib.dll
    G = _base_group()
    n_a = len(G.queries[0][1])
    a = G.queries[0][1]
    tlen, qlen = len(G.seqs[1]), len(G.seqs[2])
    _refused(dll, G, "region 0: outside its query's anchors", regions=[(0, 1, n_a)])
    _refused(dll, G, "region 0: outside its query's anchors", regions=[(0, -1, 3)])
    _refused(dll, G, "region 1: outside its query's anchors", regions=[(0, 0, 3), (0, n_a, 1)])
    _refused(dll, G, "region 0: cnt below 0", regions=[(0, 0, -1)])
    _refused(dll, G, "region 0: query index outside the call", regions=[(1, 0, 3)])
    _refused(dll, G, "anchor 5 of query 0: target id outside the group", queries=_with_anchor(G, 5, x=int(a[5, 0]) | 2 << 32))
    _refused(dll, G, "anchor 5 of query 0: position outside its sequence", queries=_with_anchor(G, 5, x=int(a[5, 0]) & ~0xffffffff | tlen))
    _refused(dll, G, "anchor 0 of query 0: position outside its sequence", queries=_with_anchor(G, 0, x=int(a[0, 0]) & ~0xffffffff | 6))      # position minus k/2 below 0
    _refused(dll, G, "anchor 7 of query 0: position outside its sequence", queries=_with_anchor(G, 7, y=int(a[7, 1]) & ~0xffffffff | qlen))
    _refused(dll, G, "anchor 0 of query 0: position outside its sequence", queries=_with_anchor(G, 0, y=int(a[0, 1]) & ~0xffffffff | 6))
    _refused(dll, G, "anchor 3 of query 0: position outside its sequence", queries=_with_anchor(G, 3, y=int(a[3, 1]) | 0x80000000))         # a negative position
    _refused(dll, G, "region 0: non-monotone chain", queries=_with_anchor(G, 9, x=int(a[8, 0])))                                           # the target stands still
    _refused(dll, G, "region 0: non-monotone chain", queries=_with_anchor(G, 9, y=int(a[7, 1])))                                           # the query steps back
    _refused(dll, G, "region 0: non-monotone chain", queries=_with_anchor(G, 9, x=int(a[9, 0]) | 1 << 63))                                 # the strand changes
    _refused(dll, G, "g_max outside [0, 4096]", params=dict(g_max=4097))
    _refused(dll, G, "g_max outside [0, 4096]", params=dict(g_max=-1))
    _refused(dll, G, "k below 1 or min_cnt below 0", params=dict(min_cnt=-1))


def test_cnt_zero_is_valid(gpu_lib):
    G = _base_group()
    R = pb.product_plan(gpu_lib.dll, G, regions=[(0, 5, 0)])
    assert R["out"][0].tolist() == [3] + [0] * 20 and len(R["items"][0]) == 0 and np.array_equal(R["anchors"][0], G.queries[0][1])


def test_g_max_is_an_argument(gpu_lib, monkeypatch):
    """the tap takes g_max as given and does not read PGA_PLAN_G_MAX"""
    monkeypatch.setenv("PGA_PLAN_G_MAX", "0")
    G = next(g for g in pcs.family("cap") if g.name == "cap_9_of_8")
    assert pb.product_plan(gpu_lib.dll, G, params=dict(g_max=9))["out"][0, 0] == 0
    assert pb.product_plan(gpu_lib.dll, G)["out"][0, 0] == 2
