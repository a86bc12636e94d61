"""The cases of tests/seed_cases.py and tests/sketch_cases.py on the reference alone (no device): every pin a case carries -- the branch it was
built to reach -- is asserted on what the reference's own code answers (tests/seedbind.py: expected), the ctypes mirrors are held against the
header, and the sketch cases hold between mm_sketch and the oracle's pgo_sketch.  No case is skipped or left out of a parametrisation.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import seed_cases as scs
import seedbind as sb
import sketch_cases as skc
import stagebind as stb
from conftest import ROOT


@pytest.fixture(scope="module", autouse=True)
def _shim():
    sb.ref_seed_dll()                                                           # skips only where oracle/_ref/ was not built


def pin_failures(B):
    E = sb.expected(B)
    P, bad = B.pins, []

    def want(what, got, exp):
        if got != exp:
            bad.append(f"{what}: reference {got}, pinned {exp}")
    if "raw" in P:
        want("raw", E["raw"], P["raw"])
    if "mid_occ" in P:
        want("mid_occ", E["mid_occ"], P["mid_occ"])
    for s, c in P.get("counts", {}).items():
        st = E["state"][s] & 3
        want(f"counts[{s}]", (int((st == 0).sum()), int((st == 1).sum()), int((st == 2).sum())), tuple(c))
    for s, u in P.get("used", {}).items():
        want(f"used[{s}]", np.nonzero((E["state"][s] & 3) == 1)[0].tolist(), list(u))
    for s, t in P.get("tandem", {}).items():
        want(f"tandem[{s}]", int(((E["state"][s] & 4) != 0).sum()), t)
    for s, v in P.get("rep_len", {}).items():
        want(f"rep_len[{s}]", E["rep_len"][s], v)
    for s, v in P.get("n_anchors", {}).items():
        want(f"n_anchors[{s}]", len(E["anchors"][s]), v)
    for s, v in P.get("n_self", {}).items():
        want(f"n_self[{s}]", int(((E["anchors"][s][:, 1] & np.uint64(sb.SEED_SELF)) != 0).sum()), v)
    for s, v in P.get("n_rev", {}).items():
        want(f"n_rev[{s}]", int((E["anchors"][s][:, 0] >> np.uint64(63)).sum()), v)
    if "tie" in P:
        want("tie", [s for s in range(B.n_seq) if sb.has_tie(E["anchors"][s])], list(P["tie"]))
    R = sb.expected_routes(B, E)
    for r, v in P.get("routes", {}).items():
        want(f"routes[{r}]", R[r], v)
    return bad


@pytest.mark.parametrize("fam", list(scs.FAMILIES))
def test_pins_hold_on_the_reference(fam):
    cases = scs.family(fam)
    assert len(cases) >= 20 or fam == "random"
    bad = [f"{B.name}: " + "; ".join(d) for B in cases for d in [pin_failures(B)] if d]
    assert not bad, f"{len(bad)} of {len(cases)} cases miss their pins:\n" + "\n".join(bad)
    assert len(set(B.name for B in cases)) == len(cases)


def test_every_listed_branch_is_pinned():
    """the families carry the pins the issue lists, none dropped: by name"""
    names = [B.name for f in scs.FAMILIES for B in scs.family(f)]
    for frag in ["n_keys=%d" % n for n in (4999, 5000, 5001, 9999, 10000, 10001, 15000, 15001)] + ["raw=%d" % r for r in (1021, 1022, 1023, 5000)] + \
            ["big_count_above_answer", "resolved_and_unresolved", "clamp raw=49", "clamp raw=50", "clamp raw=51", "clamp raw=499", "clamp raw=500", "clamp raw=501",
             "min=50 max=40", "empty_group", "boundary_at_key=2047", "boundary_at_key=2048", "boundary_at_key=2049", "first_key_of_another_group", "mid_occ/explicit",
             "flt/n_mv=mid_occ", "flt/n_mv=mid_occ+1", "flt/copies=mid_occ", "flt/copies=mid_occ+1", "flt/frac n_mv=700", "flt/frac=0", "frequent_in_group_only",
             "two_keys", "query_loses_all", "batch_loses_all", "batch_loses_none", "one_seed quota", "one_seed occ_dist=0", "one_seed max_max_occ",
             "span=250", "span=251", "span=750", "span=751", "streak_at_start", "streak_at_end", "streaks_one_low_apart", "heap_ties", "span=64250", "span=64251",
             "count=4095", "count=4096", "sel/rep_len", "flag=0x1", "flag=0x2", "flag=0x100000", "flag=0x200000", "flag=0x3", "group_of_one", "anchor/names",
             "reverse_first_and_last", "anchor/tandem", "equal_x_two_seeds", "empty_queries", "equal_x_across_queries", "n=2 len=65535", "n=3 len=65536",
             "n=256 len=65537", "n=257 len=65535", "three_groups_same_hashes", "300_groups_k=28", "own_mask", "random/39"]:
        assert any(frag in n for n in names), frag


def test_mid_occ_steps_where_double_arithmetic_on_the_float_fraction_puts_them():
    """index.c:204 computes (1. - f) * n in double with f a float: the answer steps to the next count at 5001, 10001 and 15001 keys and not one key
    earlier (the fraction as a float lies just below 2e-4, so the product at 5000 keys lies just above 4999)."""
    got = {}
    for B in scs.family("mid_occ"):
        if "n_keys=" in B.name:
            got[int(B.name.split("=")[1])] = sb.expected(B)["raw"][0]
    assert got == {4999: 61, 5000: 61, 5001: 59, 9999: 59, 10000: 59, 10001: 57, 15000: 57, 15001: 55}
    # (uint32)((1. - (double)f) * n) with f = 2e-4f: the last index at 4999 and 5000 keys (index 4999 at 5000), the one before it at 5001
    assert [n - 1 - scs.ref_index_kk(n) for n in (4999, 5000, 5001, 10000, 10001, 15000, 15001)] == [0, 0, 1, 1, 2, 2, 3]


def test_float_product_decides_the_query_filter_at_a_multiple_of_100():
    """seed.c:17 compares cnt with n * q_occ_frac in float: at n = 700 the product rounds to 7.0 and seven copies stay; the cases on both sides of
    every product are there and at least one multiple of 100 differs from exact arithmetic on 0.01f"""
    by = {B.name: B for B in scs.family("query_filter")}
    B = by["flt/frac n_mv=700 copies=7"]
    assert (sb.expected(B)["state"][0] & 3 == 0).sum() == 0
    B = by["flt/frac n_mv=700 copies=8"]
    assert (sb.expected(B)["state"][0] & 3 == 0).sum() == 8
    f = np.float32(0.01)
    assert any((np.float32(n) * f >= n // 100) != (n * float(f) >= n // 100) for n in (300, 700, 1100, 1500, 1900))


def test_random_batches_cross_mid_occ():
    """the random family reaches both sides of every decision somewhere: dropped, used and filtered minimizers, tandem seeds, tied and untied
    queries, empty queries, self anchors, both strands"""
    seen = dict(dropped=0, used=0, filtered=0, tandem=0, tied=0, untied=0, empty=0, self_=0, rev=0, fwd=0, groups=set(), mid=set())
    for B in scs.family("random"):
        E = sb.expected(B)
        seen["groups"].add(B.n_grp)
        seen["mid"].update(E["mid_occ"])
        for s in range(B.n_seq):
            st, a = E["state"][s], E["anchors"][s]
            seen["dropped"] += int((st & 3 == 0).sum()); seen["used"] += int((st & 3 == 1).sum()); seen["filtered"] += int((st & 3 == 2).sum())
            seen["tandem"] += int((st & 4 != 0).sum())
            seen["tied" if sb.has_tie(a) else "untied"] += 1
            seen["empty"] += len(a) == 0
            seen["self_"] += int(((a[:, 1] & np.uint64(sb.SEED_SELF)) != 0).sum())
            seen["rev"] += int((a[:, 0] >> np.uint64(63)).sum()); seen["fwd"] += int((a[:, 0] >> np.uint64(63) == 0).sum())
    assert len(scs.family("random")) == 40
    assert seen["groups"] == {1, 2, 3, 4, 5} and len(seen["mid"]) >= 3
    assert all(seen[k] > 0 for k in ("dropped", "used", "filtered", "tandem", "tied", "untied", "empty", "self_", "rev", "fwd")), seen


def test_stable_order_is_a_permutation_inside_equal_keys():
    """what mode 1 is held to: the same anchors, sorted by x, equal x in generation order"""
    n = 0
    for fam in ("anchors", "random"):
        for B in scs.family(fam):
            for a in sb.expected(B)["anchors"]:
                s = sb.stable_order(a)
                assert np.array_equal(s[:, 0], a[:, 0])
                assert sorted(map(tuple, s.tolist())) == sorted(map(tuple, a.tolist()))
                n += int(not np.array_equal(s, a))
    assert n > 0                                                                 # somewhere the reference's arrangement is not the stable one


def test_param_record_mirrors_the_header(tmp_path):
    """include/pga_align.h itself against the ctypes mirror of pga_seed_params_t: size and the offset of every field; the route counters' number"""
    ct = sb.pga_seed_params_t
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {', '  printf("%zu", sizeof(pga_seed_params_t));']
    lines += [f'  printf(" %zu", offsetof(pga_seed_params_t, {f[0]}));' for f in ct._fields_]
    lines += ['  printf(" %d\\n", PGA_N_FRONT_ROUTES);', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert got == [str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_] + [str(len(sb.ROUTES))]
    assert C.sizeof(sb.mm_seed_t) == 24 and C.sizeof(stb.mm128_t) == 16


# ---------------------------------------------------------------- sketch cases: mm_sketch against the oracle's restatement
@pytest.mark.parametrize("fam", list(skc.FAMILIES))
def test_sketch_cases_reference_vs_oracle(fam, ref_lib, oracle_lib):
    cases = skc.family(fam)
    assert cases
    n = 0
    for S in cases:
        want = [skc.ref_minimizers(ref_lib.dll, seq, S.w, S.k, i) for i, seq in enumerate(S.seqs)]
        got = [skc.oracle_minimizers(oracle_lib.dll, seq, S.w, S.k, i) for i, seq in enumerate(S.seqs)]
        assert got == want, S.name
        n += sum(len(m) for m in want)
        for i, c in S.pins.get("n_mz", {}).items():
            assert len(want[i]) == c, (S.name, i, len(want[i]))
        kern, _, lo, hi = skc.expected_routes(S, want)
        if "kernel" in S.pins:
            assert kern == S.pins["kernel"], (S.name, kern)
        if "retries" in S.pins:
            assert lo == hi == S.pins["retries"], (S.name, lo, hi)
    assert n > 0 or fam == "empty"


def test_sketch_kernel_table_follows_the_stated_conditions():
    """the kernel a (w, k) pair is pinned to, from the conditions sketch_all states: odd k, w + k <= 64 and w <= 63 for the tile kernels; eight
    positions per thread with w = 19 or 10 and a 2k + 13 bit key"""
    for (w, k), kern in skc.KERNEL.items():
        fast = k % 2 == 1 and w + k <= 64 and w <= 63
        fit8 = 2 * k + 13 <= 64 and 8 * ((w + 7) // 8) + w + k <= 96
        assert kern == ("sk_serial" if not fast else "sk_tiles8_19" if fit8 and w == 19 else "sk_tiles8_10" if fit8 and w == 10 else "sk_tiles"), (w, k)
    assert len(set(skc.KERNEL.values())) == 4
