"""The cases of tests/plan_cases.py on the reference alone (no device): every pin a case carries is asserted on what the reference's own code
produces for it, the two routes through that code (the trace of mm_align1's DP calls; mm_fix_bad_ends and the seed filters called directly) must
agree before either is trusted, the ctypes mirrors are held to pga_plan.h, and the numpy probe is checked on hand-written windows.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import plan_cases as pcs
import planbind as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY_NAMES = list(pcs.FAMILIES)


@pytest.fixture(scope="module", autouse=True)
def _shim():
    pb.ref_plan_dll()                                                           # skips only where oracle/_ref/ was not built


def region_flags(G, E, r, bit):
    """chain indices (relative to as) of region r whose anchors gained the flag `bit`"""
    j, as_, cnt = G.regions[r]
    before, after = G.queries[j][1], E["anchors"][j]
    gained = (after[as_:as_ + cnt, 1] & ~before[as_:as_ + cnt, 1]) & np.uint64(bit)
    return set(int(i) for i in np.nonzero(gained)[0])


def check_pins(G):
    E = pb.expected(G)
    for (r, f), v in G.pins.get("out", {}).items():
        got = int(E["out"][r, pb.OUT_FIELDS.index(f)])
        assert got == v, f"{G.name}: region {r}: the reference gives {f} = {got}, the case was built for {v}"
    for r, want in G.pins.get("ignore", {}).items():
        assert region_flags(G, E, r, pb.A_IGNORE) == want, f"{G.name}: region {r}: IGNORE at {sorted(region_flags(G, E, r, pb.A_IGNORE))}, built for {sorted(want)}"
    for r, want in G.pins.get("join", {}).items():
        assert region_flags(G, E, r, pb.A_LONG_JOIN) == want, f"{G.name}: region {r}: LONG_JOIN at {sorted(region_flags(G, E, r, pb.A_LONG_JOIN))}, built for {sorted(want)}"
    for r, want in G.pins.get("segs", {}).items():
        if want is not None:
            got = len(E["regions"][r]["trace"]["segs"])
            assert got == want, f"{G.name}: region {r}: the reference cuts {got} segments, built for {want}"
    for r, want in G.pins.get("items", {}).items():
        got = [(int(x[0]), int(x[6]), int(x[7])) for x in E["items"][r]]
        assert got == list(want), f"{G.name}: region {r}: items (kind, bw1, m) {got[:12]} ..., built for {list(want)[:12]} ..."


def check_routes_agree(G):
    """the trace-derived plan against the direct wrappers: as1 / cnt1 and every anchor word"""
    E = pb.expected(G)
    direct = [a.copy() for _, a in G.queries]
    p = G.par()
    for r, (j, as_, cnt) in enumerate(G.regions):
        info = E["regions"][r]
        if info["status"] != 0:
            continue
        qlen = len(G.seqs[G.queries[j][0]])
        as1, cnt1 = pb.ref_trim_and_filter(qlen, direct[j], as_, cnt, p)
        t = info["trace"]
        if t is not None:
            assert (t["as1"], t["cnt1"]) == (as1, cnt1), f"{G.name}: region {r}: trace gives as1, cnt1 = {t['as1']}, {t['cnt1']}, mm_fix_bad_ends {as1}, {cnt1}"
    for j in range(len(G.queries)):
        assert np.array_equal(direct[j], E["anchors"][j]), f"{G.name}: query {j}: the flags after mm_align1 differ from the flags after the filters called directly"


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_pins_on_reference(fam):
    for G in pcs.family(fam):
        check_pins(G)


@pytest.mark.parametrize("fam", FAMILY_NAMES)
def test_trace_agrees_with_direct_wrappers(fam):
    for G in pcs.family(fam):
        check_routes_agree(G)


def test_random_groups_complete():
    """the reference trace completes, with no assert, for all forty random groups; every region is planned (none over the cap) and the groups
    exercise both probe answers"""
    kinds = set()
    groups = pcs.family("random")
    assert len(groups) == pcs.N_RANDOM == 40
    for G in groups:
        E = pb.expected(G)
        assert 3 <= len(G.regions) <= 6
        assert (E["out"][:, 0] == 0).all(), f"{G.name}: statuses {E['out'][:, 0]}"
        for it in E["items"]:
            kinds.update(int(k) for k in it[:, 0])
    assert kinds == {0, 1, 2}


def test_case_inventory():
    for cnt in pcs.EXTENT_CNT:
        assert any(g.name.startswith(f"extent_cnt{cnt}_") for g in pcs.family("extent"))
    names = {g.name for f in FAMILY_NAMES for g in pcs.family(f)}
    assert len(names) == sum(len(pcs.family(f)) for f in FAMILY_NAMES)
    for G in (g for f in FAMILY_NAMES if f != "random" for g in pcs.family(f)):
        assert G.pins or G.name == "host_empty_list", f"{G.name} carries no pin"
        assert G.base == 1 and len(G.seqs[0]) % 16 != 0                         # nothing at offset 0 of the store, nothing word-aligned by accident


# ---------------------------------------------------------------- the struct mirrors
def _c_struct(text, name):
    m = re.search(r"struct " + name + r" \{(.*?)\n\};", text, re.S)
    assert m, name
    body = re.sub(r"//[^\n]*", "", m.group(1))
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        for nm in rest.split(","):
            nm = nm.strip()
            k = re.match(r"(\w+)\[(\d+)\]", nm)
            fields.append((k.group(1), ty, int(k.group(2))) if k else (nm, ty, 1))
    return fields


_CT = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, "uint64_t": C.c_uint64}


@pytest.mark.parametrize("name,mirror", [("PlanParams", pb.PlanParams), ("PlanOut", pb.PlanOut), ("PlanItem", pb.PlanItem), ("PlanIn", pb.PlanIn)])
def test_struct_mirrors(name, mirror):
    """field names, types, order, offsets and size against pga_plan.h (natural alignment, as the compiler lays plain integer records out)"""
    text = open(os.path.join(ROOT, "pangraph_amd", "csrc", "pga_plan.h")).read()
    off = 0
    fields = _c_struct(text, name)
    assert len(fields) == len(mirror._fields_)
    for (nm, ty, n), (pn, pt) in zip(fields, mirror._fields_):
        ct = _CT[ty] * n if n > 1 else _CT[ty]
        assert pn.rstrip("_") == nm and C.sizeof(pt) == C.sizeof(ct), (name, nm, pn)
        al = C.sizeof(_CT[ty])
        off = (off + al - 1) // al * al
        assert getattr(mirror, pn).offset == off, (name, nm)
        off += C.sizeof(ct)
    assert C.sizeof(mirror) == (off + 7) // 8 * 8 if any(C.sizeof(_CT[t]) == 8 for _, t, _ in fields) else off
    # and the C mirrors of include/pga_align.h name the same fields in the same order
    h = open(os.path.join(ROOT, "include", "pga_align.h")).read()
    if name != "PlanIn":
        cname = {"PlanParams": "pga_region_params_t", "PlanOut": "pga_region_out_t", "PlanItem": "pga_region_item_t"}[name]
        m = re.search(r"typedef struct \{([^}]*)\} " + cname + ";", h, re.S)
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        names = [re.sub(r"\[\d+\]", "", w.strip()) for d in body.split(";") if d.strip() for w in d.strip().split(None, 1)[1].split(",")]
        assert names == [nm for nm, _, _ in fields]


def test_extent_and_item_views():
    assert C.sizeof(pb.PlanOut) == 4 * len(pb.OUT_FIELDS) and C.sizeof(pb.PlanItem) == 48 and C.sizeof(pb.PlanParams) == 64 and C.sizeof(pb.PlanIn) == 48


# ---------------------------------------------------------------- the numpy probe on hand-written windows
def test_numpy_probe():
    t = np.array([0, 1, 2, 3, 0, 1, 2, 3], np.uint8)
    assert pb.probe(t, t, 0) == 0
    q = t.copy()
    q[0] = 3
    assert pb.probe(t, q, 0) == -1 and pb.probe(t, q, 1) == 1
    q[7] = 0
    assert pb.probe(t, q, 1) == -1 and pb.probe(t, q, 2) == 2
    n = t.copy()
    n[7] = 4
    assert pb.probe(t, n, 8) == -1 and pb.probe(n, t, 8) == -1 and pb.probe(n, n, 8) == -1
    assert pb.probe(t[:0], t[:0], 0) == 0
    # a reverse-strand query: the aligned strand is the complemented, reversed forward query
    fwd = np.array([3, 3, 0, 1, 4], np.uint8)
    assert list(pb.revcomp(fwd)) == [4, 2, 3, 0, 0]
    assert pb.probe(np.array([2, 3, 0, 0], np.uint8), pb.revcomp(fwd)[1:], 0) == 0


def test_collapse_by_hand():
    t = np.zeros(40, np.uint8)
    q = t.copy()
    q[[12, 13, 14]] = 1                                                          # three mismatches in the second of four segments of ten
    q[35] = 1
    segs = [dict(i=k + 1, i_prev=k, rs=10 * k, qs=10 * k, re=10 * k + 10, qe=10 * k + 10, bw1=100) for k in range(4)]
    it = pb.collapse(segs, t, q, dict(probe_m_max=2, max_sw_mat=0))
    assert it.tolist() == [[0, 1, 0, 0, 10, 10, 1, 0, 0], [2, 2, 10, 10, 20, 20, 100, 0, 1], [0, 4, 20, 20, 40, 40, 2, 1, 2]]
    segs[0]["bw1"] = 9                                                           # a band below the length: not eligible, kind 1
    assert pb.collapse(segs, t, q, dict(probe_m_max=2, max_sw_mat=0))[0].tolist() == [1, 1, 0, 0, 10, 10, 9, 0, 0]
    assert (pb.collapse(segs[1:], t, q, dict(probe_m_max=2, max_sw_mat=99))[:, 0] == 2).all()      # 10 x 10 above max_sw_mat: never probed
