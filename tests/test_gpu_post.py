"""The post-DP kernels of pangraph_amd/csrc/pga_post.hip, each through its own tap and compared exactly with a CPU authority:

  k_cigar_finish   pga_stage_post_finish   the reference's mm_update_extra (oracle/ref_align_shim.c): all eleven PostFinRes fields and the final list
  k_zdrop_walk     pga_stage_post_walk     pgo_zdrop_walk (pinned on the reference's mm_test_zdrop in tests/test_post_cases_cpu.py)
  k_seg_identity   pga_stage_post_identity a numpy count

on the cases of tests/post_cases.py, whose pins tests/test_post_cases_cpu.py asserts on the reference alone.  Every finish case runs under every
scoring, on both strands and at the offsets of post_cases.VARIANTS; nothing is sampled and there is no tolerance.  One call per family, scoring
and variant, so a failure names its family; the first request of a call sits at base 0 of the store.
"""
import numpy as np
import pytest

import post_cases as pc
import postbind as pb

pytestmark = pytest.mark.gpu

CASES = pc.all_cases()
BY_FAMILY = {f: [c for c in CASES if c.family == f] for f in pc.FAMILIES}
SC_IDS = ["a%d_b%d_q%d_e%d" % s for s in pc.SCORINGS]
_PAD = np.random.default_rng(4242).integers(0, 5, 64).astype(np.uint8)          # what surrounds an embedded window (N included)


@pytest.fixture(scope="module", autouse=True)
def _shim():
    pb.ref_align_dll()                                                           # skips only where oracle/_ref/ was not built


def embed(case, variant, cigar=None):
    """a request (forward query, q_start, q_rev, target, t_start, list) for a case under a variant of post_cases.VARIANTS"""
    q_rev, ql, qr, tl, tr = variant
    aligned = np.concatenate([_PAD[:ql], case.q, _PAD[20:20 + qr]])
    fwd = pb.revcomp(aligned) if q_rev else aligned
    tgt = np.concatenate([_PAD[30:30 + tl], case.t, _PAD[7:7 + tr]])
    return (fwd, ql, q_rev, tgt, tl, case.cigar if cigar is None else cigar)


def check_finish(dll, cases, variant, sc, what):
    res, lists = pb.product_post_finish(dll, [embed(c, variant) for c in cases], sc)
    exp = [pb.finish_expected(c, sc) for c in cases]
    want = np.stack([e["res"] for e in exp])
    if not np.array_equal(res, want):
        i = int(np.nonzero((res != want).any(axis=1))[0][0])
        diff = {f: (int(res[i, k]), int(want[i, k])) for k, f in enumerate(pb.FIN_FIELDS) if res[i, k] != want[i, k]}
        raise AssertionError(f"{what}: request {i} ({cases[i].name}, {pc.cigstr(cases[i].cigar)[:80]}) (device, reference): {diff}; "
                             f"{int((res != want).any(axis=1).sum())} of {len(cases)} requests differ")
    for i, (got, e) in enumerate(zip(lists, exp)):
        assert np.array_equal(got, e["cigar"]), f"{what}: request {i} ({cases[i].name}): final list {pc.cigstr(got)[:120]}, reference {pc.cigstr(e['cigar'])[:120]}"


@pytest.mark.parametrize("sc", pc.SCORINGS, ids=SC_IDS)
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_finish_family(family, sc, gpu_lib):
    for v in pc.VARIANTS:
        check_finish(gpu_lib.dll, BY_FAMILY[family], v, sc, f"{family} {sc} variant {v}")


@pytest.mark.parametrize("sc", pc.SCORINGS, ids=SC_IDS)
def test_finish_first_in_store(sc, gpu_lib):
    """q_rev = 1 and a match run that ends on forward position 0..14 of the query: as request 0 (q_off == 0: the branch that reads base by base)
    and again as request 1 (q_off >= 16: the sixteen-base read reaches below the query's first base)"""
    for c in BY_FAMILY["first_in_store"] + BY_FAMILY["leading"][:2]:
        for r in range(15):
            check_finish(gpu_lib.dll, [c, c], (1, 3, r, 2, 1), sc, f"first in store, {r} bases behind the window")


@pytest.mark.parametrize("sc", pc.SCORINGS, ids=SC_IDS)
@pytest.mark.parametrize("name", ("batch_4097", "batch_8200"))
def test_finish_batches(name, sc, gpu_lib):
    """over 4096 requests the launcher leaves the pinned-memory route; over 8192 a wave takes a second region into the LDS it has used"""
    batch = pc.batches()[name]
    for v in pc.VARIANTS:
        check_finish(gpu_lib.dll, batch, v, sc, f"{name} {sc} variant {v}")


def test_finish_long_list_behind_short_ones(gpu_lib):
    """8192 tiny requests and then the long lists: each long list runs on a wave that has finished a tiny region, the in-place ones beside LDS ones"""
    batch = pc.batches()["batch_8200"][:8192] + BY_FAMILY["long_lists"]
    check_finish(gpu_lib.dll, batch, pc.VARIANTS[3], pc.SCORINGS[1], "long lists behind 8192 tiny requests")


# ------------------------------------------------------------------------------------------------ the z-drop walk
def check_walk(dll, oracle_dll, cases, variant, sc, what):
    res = pb.product_post_walk(dll, [embed(c, variant) for c in cases], sc)
    want = np.array([pb.oracle_zdrop_walk(oracle_dll, c.q, c.t, c.cigar, sc) for c in cases], np.int32).reshape(len(cases), 5)
    if not np.array_equal(res, want):
        i = int(np.nonzero((res != want).any(axis=1))[0][0])
        raise AssertionError(f"{what}: request {i} ({cases[i].name}) {pb.WALK_FIELDS}: device {res[i].tolist()}, restatement {want[i].tolist()}; "
                             f"{int((res != want).any(axis=1).sum())} of {len(cases)} differ")


@pytest.mark.parametrize("sc", pc.SCORINGS, ids=SC_IDS)
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_walk_family(family, sc, gpu_lib, oracle_lib):
    """the same sequences and lists, before fixing"""
    for v in pc.VARIANTS:
        check_walk(gpu_lib.dll, oracle_lib.dll, BY_FAMILY[family], v, sc, f"walk {family} {sc} variant {v}")


@pytest.mark.parametrize("name", ("batch_4097", "batch_8200"))
def test_walk_batches(name, gpu_lib, oracle_lib):
    batch = pc.batches()[name]
    for sc, v in zip(pc.SCORINGS, pc.VARIANTS + pc.VARIANTS[:1]):
        check_walk(gpu_lib.dll, oracle_lib.dll, batch, v, sc, f"walk {name} {sc} variant {v}")


# ------------------------------------------------------------------------------------------------ identity probes
def probe_req(t, q, q_rev, ql, qr, tl):
    aligned = np.concatenate([_PAD[:ql], q, _PAD[20:20 + qr]])
    return (pb.revcomp(aligned) if q_rev else aligned, ql, q_rev, np.concatenate([_PAD[30:30 + tl], t, _PAD[:3]]), tl, len(t))


def count(t, q, m_max):
    """the probe's answer as numpy counts it"""
    if ((t > 3) | (q > 3)).any():
        return -1
    m = int((t != q).sum())
    return m if m <= m_max else -1


@pytest.mark.parametrize("q_rev", (0, 1))
def test_identity_probes(q_rev, gpu_lib):
    probes = pc.probe_cases()
    for ql, qr, tl in ((0, 0, 0), (5, 9, 33), (16, 0, 1)):
        got = pb.product_post_identity(gpu_lib.dll, [probe_req(t, q, q_rev, ql, qr, tl) for _, t, q, _ in probes], pc.PROBE_M_MAX)
        for (name, t, q, want), g in zip(probes, got.tolist()):
            assert want == count(t, q, pc.PROBE_M_MAX), f"{name}: the generator's own expectation"
            assert g == want, f"{name} (q_rev {q_rev}, offsets {ql}, {tl}): device {g}, numpy {want}"
    kinds = [w for _, _, _, w in probes]
    assert kinds.count(0) >= 6 and kinds.count(pc.PROBE_M_MAX) >= 5 and kinds.count(-1) >= 20


@pytest.mark.parametrize("q_rev", (0, 1))
def test_identity_probe_batch_wraps_the_grid(q_rev, gpu_lib):
    """33 000 probes on a grid of 32 768 waves: the last ones are a wave's second probe; beyond 4096 the launcher uses device buffers"""
    t, q = pc.probe_batch()
    assert len(t) > 32_768
    m_max = 2
    fwd = np.ascontiguousarray(np.where(q < 4, 3 - q, 4).astype(np.uint8)[:, ::-1]) if q_rev else q      # row-wise reverse complement
    got = pb.product_post_identity(gpu_lib.dll, [(fwd[i], 0, q_rev, t[i], 0, 8) for i in range(len(t))], m_max)
    amb = ((t > 3) | (q > 3)).any(axis=1)
    m = (t != q).sum(axis=1)
    want = np.where(amb | (m > m_max), -1, m).astype(np.int32)
    assert np.array_equal(got, want), f"{int((got != want).sum())} probes differ, the first at {int(np.nonzero(got != want)[0][0])}"
    assert (want == -1).sum() > 100 and (want > 0).sum() > 1000 and (want[32_768:] >= 0).any() and (want[32_768:] == -1).any()
