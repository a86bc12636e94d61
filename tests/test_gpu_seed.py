"""The stages between sketching and chaining (pga_index.hip: build_index_ex and index_cal_max_occ with pga_maxocc_hist.h; pga_seed.hip: seed_all and
seed_exact_order; the host's group_mid_occ) through their tap pga_stage_seed, compared exactly with the reference's own code (tests/seedbind.py:
expected) on the cases of tests/seed_cases.py, whose pins tests/test_seed_cases_cpu.py asserts on the reference alone.  Every mid_occ, every
minimizer's state, every rep_len, every anchor offset and every anchor word, in both modes; the route counters prove which branch answered.
Nothing is sampled and there is no tolerance.
"""
import copy

import numpy as np
import pytest

import seed_cases as scs
import seedbind as sb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _shim():
    sb.ref_seed_dll()                                                           # skips only where oracle/_ref/ was not built


def differences(B, R, E, mode):
    """what the device's answer R for batch B differs in from the reference's E, as a list of strings (empty: identical)"""
    bad = []
    if R["mid_occ"] != E["mid_occ"]:
        bad.append(f"mid_occ {R['mid_occ']} against {E['mid_occ']}")
    if R["rep_len"] != E["rep_len"]:
        d = [(s, R["rep_len"][s], E["rep_len"][s]) for s in range(B.n_seq) if R["rep_len"][s] != E["rep_len"][s]]
        bad.append(f"rep_len (sequence, device, reference): {d[:4]}")
    for s in range(B.n_seq):
        got, want = R["state"][s], E["state"][s]
        if not np.array_equal(got, want):
            i = int(np.nonzero(got != want)[0][0])
            bad.append(f"sequence {s}: {int((got != want).sum())} minimizer states differ, the first at {i}: {int(got[i])} against {int(want[i])}")
        got, want = R["anchors"][s], E["anchors"][s] if mode == 0 else sb.stable_order(E["anchors"][s])
        if got.shape != want.shape:
            bad.append(f"query {s}: {len(got)} anchors, reference {len(want)}")
        elif not np.array_equal(got, want):
            i = int(np.nonzero((got != want).any(axis=1))[0][0])
            bad.append(f"query {s}: {int((got != want).any(axis=1).sum())} anchors differ, the first at {i}: {int(got[i, 0]):#x} {int(got[i, 1]):#x} "
                       f"against {int(want[i, 0]):#x} {int(want[i, 1]):#x}")
        tie = int(sb.has_tie(E["anchors"][s])) if mode == 1 else 0
        if int(R["q_tie"][s] != 0) != tie:
            bad.append(f"query {s}: q_tie {R['q_tie'][s]}, expected {tie}")
    return bad


def check_batches(dll, batches, mode):
    bad = []
    for B in batches:
        E = sb.expected(B)
        sb.product_front_routes(dll)
        R = sb.product_seed(dll, B, mode)
        routes = sb.product_front_routes(dll)
        d = differences(B, R, E, mode)
        want = sb.expected_routes(B, E)
        if mode == 1:
            want["replay_q"] = 0                                                 # a batch asks for the reference's order later, where chaining needs it
        got = {r: routes[r] for r in want}
        if got != want:
            d.append(f"route counters {got}, expected {want}")
        if any(routes[r] for r in ("sk_tiles8_19", "sk_tiles8_10", "sk_tiles", "sk_serial", "sk_retry")):
            d.append(f"the tap sketched: {routes}")
        if d:
            bad.append(f"{B.name}: " + "; ".join(d[:4]))
    assert not bad, f"{len(bad)} of {len(batches)} cases differ from the reference:\n" + "\n".join(bad[:12])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("fam", [f for f in scs.FAMILIES if f != "random"])
def test_family(fam, mode, gpu_lib):
    check_batches(gpu_lib.dll, scs.family(fam), mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("part", range(2))
def test_random_batches(part, mode, gpu_lib):
    check_batches(gpu_lib.dll, scs.family("random")[part::2], mode)


def test_mode_1_is_mode_0_as_a_multiset_and_stable(gpu_lib):
    """per query the stable order holds the anchors of the reference's order, sorted by x, and equal x lie in raw (generation) order: ascending
    query position on the forward strand, descending on the reverse strand"""
    n_tied = 0
    for B in scs.family("anchors") + scs.family("random")[:10]:
        R0, R1 = sb.product_seed(gpu_lib.dll, B, 0), sb.product_seed(gpu_lib.dll, B, 1)
        for s in range(B.n_seq):
            a0, a1 = R0["anchors"][s], R1["anchors"][s]
            assert sorted(map(tuple, a0.tolist())) == sorted(map(tuple, a1.tolist())), (B.name, s)
            assert (np.diff(a1[:, 0].astype(object)) >= 0).all() if len(a1) > 1 else True
            assert np.array_equal(a1, sb.stable_order(a0)), (B.name, s)
            n_tied += int(R1["q_tie"][s] != 0)
    assert n_tied > 0


def test_route_counters_name_the_branches(gpu_lib):
    """the pinned routes of the cases built for them, read from the device's counters: the two-sort index, the sort route of mid_occ (and the
    histogram below it), the replay for a tie inside a query and none for equal keys across a query boundary"""
    by = {B.name: B for f in scs.FAMILIES if f != "random" for B in scs.family(f)}
    for name, want in (("anchor/300_groups_k=28", dict(idx_one_sort=0, idx_two_sorts=1)), ("mid_occ/raw=1023", dict(mo_hist=1, mo_sort=0)),
                       ("mid_occ/raw=1024", dict(mo_hist=0, mo_sort=1)), ("mid_occ/raw=5000", dict(mo_hist=0, mo_sort=1)),
                       ("mid_occ/resolved_and_unresolved", dict(mo_hist=0, mo_sort=1)), ("mid_occ/big_count_above_answer", dict(mo_hist=1, mo_sort=0)),
                       ("mid_occ/explicit", dict(mo_hist=0, mo_sort=0)), ("anchor/equal_x_two_seeds", dict(replay_q=1, idx_one_sort=1)),
                       ("anchor/equal_x_across_queries", dict(replay_q=0))):
        B = by[name]
        assert all(B.pins.get("routes", {}).get(r, v) == v for r, v in want.items()), name
        sb.product_front_routes(gpu_lib.dll)
        R = sb.product_seed(gpu_lib.dll, B, 0)
        got = sb.product_front_routes(gpu_lib.dll)
        assert {r: got[r] for r in want} == want, (name, got)
        if name == "anchor/equal_x_across_queries":
            R1 = sb.product_seed(gpu_lib.dll, B, 1)
            assert R1["q_tie"] == [0, 0, 0] and int(R["anchors"][1][-1, 0]) == int(R["anchors"][2][0, 0])
    assert sb.product_front_routes(gpu_lib.dll)["replay_q"] == 0                  # ... and reading zeroes them


# ---------------------------------------------------------------- refusals: by name, without a launch
def _valid():
    b = scs.Bld(15, 10, mid_occ=5, flag=scs.PROD)
    q, t = b.seq(300), b.seq(300)
    h = b.fresh()
    b.put(q, 20, h, 0), b.put(q, 60, b.fresh(), 1), b.put(t, 40, h, 1), b.put(t, 90, b.fresh(), 0)
    b.group()
    u = b.seq(200)
    b.put(u, 30, h, 0)
    return b.batch("refusal/base")


def _mutated(fn):
    B = copy.deepcopy(_valid())
    fn(B)
    return B


def _set(B, s, j, col, v):
    B.mz[s][j, col] = np.uint64(v)


REFUSALS = [
    ("carries rid", lambda B: _set(B, 1, 0, 1, 0 << 32 | 40 << 1 | 1)),
    ("carries rid", lambda B: _set(B, 2, 0, 1, 3 << 32 | 30 << 1)),
    ("positions do not ascend", lambda B: _set(B, 0, 1, 1, 0 << 32 | 20 << 1 | 1)),
    ("positions do not ascend", lambda B: _set(B, 0, 1, 1, 0 << 32 | 19 << 1)),
    ("is outside [k - 1, len)", lambda B: _set(B, 0, 0, 1, 0 << 32 | 13 << 1)),
    ("is outside [k - 1, len)", lambda B: _set(B, 0, 1, 1, 0 << 32 | 300 << 1)),
    ("the low byte of x is 14, not k", lambda B: _set(B, 1, 1, 0, 77 << 8 | 14)),
    ("the hash has 2k bits or more", lambda B: _set(B, 1, 1, 0, (1 << 30) << 8 | 15)),
    ("duplicate sequence name '0' inside a group", lambda B: B.names.__setitem__(1, b"0")),
    ("groups are not contiguous", lambda B: B.grp_off.__setitem__(0, 1)),
    ("groups are not contiguous", lambda B: B.grp_off.__setitem__(1, 4)),
    ("groups are not contiguous", lambda B: B.grp_off.__setitem__(2, 2)),
    ("k must be in [1,28] and w in [1,255]", lambda B: B.params.__setitem__("k", 29)),
    ("k must be in [1,28] and w in [1,255]", lambda B: B.params.__setitem__("k", 0)),
    ("k must be in [1,28] and w in [1,255]", lambda B: B.params.__setitem__("w", 0)),
    ("k must be in [1,28] and w in [1,255]", lambda B: B.params.__setitem__("w", 256)),
    ("flag holds bits other than", lambda B: B.params.__setitem__("flag", scs.PROD | 0x4)),
    ("flag holds bits other than", lambda B: B.params.__setitem__("flag", 0x80000000)),
]


@pytest.mark.parametrize("i", range(len(REFUSALS)))
def test_refusals_by_message(i, gpu_lib):
    msg, fn = REFUSALS[i]
    sb.product_seed(gpu_lib.dll, _valid(), 0)                                    # the unchanged batch is taken
    sb.product_front_routes(gpu_lib.dll)
    with pytest.raises(RuntimeError) as e:
        sb.product_seed(gpu_lib.dll, _mutated(fn), 0)
    assert msg in str(e.value), str(e.value)
    assert not any(sb.product_front_routes(gpu_lib.dll).values())                # nothing was built
    with pytest.raises(RuntimeError) as e:
        sb.product_seed(gpu_lib.dll, _valid(), 2)
    assert "mode is 0" in str(e.value)


def test_the_same_name_in_two_groups_is_taken(gpu_lib):
    B = _mutated(lambda B: B.names.__setitem__(2, b"0"))
    R, E = sb.product_seed(gpu_lib.dll, B, 0), sb.expected(B)
    assert not differences(B, R, E, 0)
