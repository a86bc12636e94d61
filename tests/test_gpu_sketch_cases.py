"""The three sketch kernels and the retry of their staging slabs (pga_sketch.hip: k_sketch_tiles8<19>, <10>, k_sketch_tiles, k_sketch_serial, sketch_all)
through the tap pga_stage_sketch on the cases of tests/sketch_cases.py, compared exactly with the reference's mm_sketch (an empty sequence expects
no minimizer: the reference asserts len > 0).  The route counters of pga_stage_front_routes name the kernel that ran and count the retries.
tests/test_seed_cases_cpu.py holds the same cases between mm_sketch and the oracle's pgo_sketch.
"""
import pytest

import seedbind as sb
import sketch_cases as skc

pytestmark = pytest.mark.gpu

SKETCH_ROUTES = ("sk_tiles8_19", "sk_tiles8_10", "sk_tiles", "sk_serial", "sk_retry")


@pytest.mark.parametrize("fam", list(skc.FAMILIES))
def test_family(fam, gpu_lib, ref_lib):
    bad = []
    cases = skc.family(fam)
    for S in cases:
        want = [skc.ref_minimizers(ref_lib.dll, seq, S.w, S.k, i) for i, seq in enumerate(S.seqs)]
        sb.product_front_routes(gpu_lib.dll)
        got = skc.product_minimizers(gpu_lib.dll, S.seqs, S.w, S.k)
        routes = sb.product_front_routes(gpu_lib.dll)
        d = []
        for i, (g, w_) in enumerate(zip(got, want)):
            if g != w_:
                j = next((j for j in range(min(len(g), len(w_))) if g[j] != w_[j]), min(len(g), len(w_)))
                d.append(f"sequence {i} (length {len(S.seqs[i])}): {len(g)} minimizers, reference {len(w_)}; first difference at {j}: "
                         f"{g[j] if j < len(g) else None} against {w_[j] if j < len(w_) else None}")
        d += skc.routes_failures(S, want, routes)
        if "kernel" in S.pins and routes[S.pins["kernel"]] == 0:
            d.append(f"{S.pins['kernel']} did not run: {routes}")
        if d:
            bad.append(f"{S.name}: " + "; ".join(d[:3]))
    assert not bad, f"{len(bad)} of {len(cases)} cases differ from the reference:\n" + "\n".join(bad[:12])


def test_every_kernel_and_both_retry_depths_ran(gpu_lib, ref_lib):
    """by counter: each of the four kernels answers one of the border pairs, and the homopolymer needs two retries of the slab with w = 19, one with
    w = 10 and w = 5"""
    ran = set()
    for S in skc.family("borders") + skc.family("repeats"):
        sb.product_front_routes(gpu_lib.dll)
        skc.product_minimizers(gpu_lib.dll, S.seqs, S.w, S.k)
        routes = sb.product_front_routes(gpu_lib.dll)
        ran |= {r for r in SKETCH_ROUTES if routes[r]}
        assert [r for r in SKETCH_ROUTES[:4] if routes[r]] == [skc.KERNEL[(S.w, S.k)]], (S.name, routes)
        if "homopolymer" in S.name:
            assert routes["sk_retry"] == (2 if S.w >= 16 else 1) and routes[skc.KERNEL[(S.w, S.k)]] == routes["sk_retry"] + 1, (S.name, routes)
    assert ran == set(SKETCH_ROUTES)
