"""The restatement of block_slice (tests/slice_ref.py) on the reference's own unit-test vectors, recorded as data in
tests/golden/slice_vectors.json (slice.rs: generate_example with both intervals, test_node_coords, test_new_position_*, test_block_slice_*);
the partition invariant of the restatement on random members; the ctypes mirrors of the slicing structs against the header.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import slice_cases as sc
import slice_ref as sr
from conftest import GOLDEN, ROOT

V = json.load(open(os.path.join(GOLDEN, "slice_vectors.json")))


@pytest.mark.parametrize("case", V["example"]["slices"], ids=lambda c: f"{c['start']}-{c['end']}")
def test_example_slices(case):
    cons, ed = V["example"]["consensus"], sc.edit_from_json(V["example"]["edit"])
    i = sr.interval(case["start"], case["end"], aligned=True)
    assert sr.slice_substitutions(i, ed["subs"]) == [tuple(x) for x in case["subs"]]
    assert sr.slice_deletions(i, ed["dels"]) == [tuple(x) for x in case["dels"]]
    assert sr.slice_insertions(i, ed["inss"], len(cons)) == [tuple(x) for x in case["inss"]]
    assert sr.interval_node_coords(i, ed, len(cons)) == tuple(case["node_coords"])


def test_node_coords():
    c = V["node_coords"]
    assert sr.interval_node_coords(sr.interval(c["start"], c["end"], aligned=True), sc.edit_from_json(c["edit"]), c["block_len"]) == tuple(c["expected"])


@pytest.mark.parametrize("c", V["new_position_circular"], ids=lambda c: f"{c['old_position']}-{'rev' if c['reverse'] else 'fwd'}")
def test_new_position_circular(c):
    assert sr.new_position_circular(tuple(c["old_position"]), tuple(c["node_coords"]), c["path_len"], c["reverse"]) == tuple(c["expected"])


@pytest.mark.parametrize("c", V["new_position_non_circular"], ids=lambda c: f"{c['old_position']}-{'rev' if c['reverse'] else 'fwd'}")
def test_new_position_non_circular(c):
    assert sr.new_position_non_circular(tuple(c["old_position"]), tuple(c["node_coords"]), c["reverse"]) == tuple(c["expected"])


@pytest.mark.parametrize("case", V["block_slice"]["cases"], ids=lambda c: c["name"])
def test_block_slice(case):
    bs = V["block_slice"]
    nodes = [(n["position"][0], n["position"][1], n["path_len"], n["reverse"], n["circular"]) for n in bs["nodes"]]
    i = sr.interval(case["start"], case["end"], case["aligned"], case["is_anchor"], case["reverse"])
    cons, kept, dropped = sr.block_slice(bs["consensus"], [sc.edit_from_json(e) for e in bs["members"]], nodes, i)
    assert cons == case["consensus"] and dropped == [] and [k["member"] for k in kept] == [0, 1, 2]
    for k, n, e in zip(kept, case["nodes"], case["edits"]):
        assert (k["reverse"], k["pos"]) == (n["reverse"], tuple(n["position"]))
        assert {f: k[f] for f in ("subs", "dels", "inss")} == sc.edit_from_json(e)


def test_empty_alignment_is_what_apply_leaves():
    cons = "ACGTACGTAC"
    assert sr.is_empty_alignment(sc.E(dels=[(0, 10)]), cons)
    assert sr.is_empty_alignment(sc.E(dels=[(0, 6), (4, 6)]), cons)                      # overlapping, together the whole slice
    assert not sr.is_empty_alignment(sc.E(dels=[(0, 6), (2, 4)]), cons)                  # lengths add up to 10, the last four letters stay
    assert not sr.is_empty_alignment(sc.E(dels=[(0, 10)], inss=[(3, "A")]), cons)
    assert not sr.is_empty_alignment(sc.E(dels=[(0, 9)]), cons)
    i0, i1 = sr.interval(0, 5), sr.interval(5, 10)
    _, kept, dropped = sr.block_slice(cons, [sc.E(dels=[(0, 5)]), sc.E()], [(0, 5, 0, False, False), (0, 10, 0, False, False)], i0)
    assert dropped == [0] and [k["member"] for k in kept] == [1]
    _, kept, dropped = sr.block_slice(cons, [sc.E(dels=[(0, 5)]), sc.E()], [(0, 5, 0, False, False), (0, 10, 0, False, False)], i1)
    assert dropped == [] and [(k["member"], k["node"], k["pos"]) for k in kept] == [(0, (0, 5), (0, 5)), (1, (5, 10), (5, 10))]


def test_the_reference_panics_are_errors():
    with pytest.raises(sr.Panic):                                                         # a reverse node that ends before its coordinates
        sr.block_slice("ACGTACGTAC", [sc.E()], [(0, 5, 0, True, False)], sr.interval(0, 10))
    with pytest.raises(sr.Panic):                                                         # two deletions over the same positions before a boundary
        sr.block_slice("ACGTACGTAC", [sc.E(dels=[(0, 3), (0, 3)])], [(0, 10, 0, False, False)], sr.interval(4, 10))
    with pytest.raises(sr.Panic):
        sr.block_slice("ACGTACGTAC", [sc.E(subs=[(10, "A")])], [(0, 10, 0, False, False)], sr.interval(4, 10))


@pytest.mark.parametrize("seed", range(6))
def test_partition_invariant(seed):
    """For intervals that tile the block, slicing is a partition of the member's sequence.  Preconditions, met by construction
    (slice_cases.random_member; no case is skipped): the deletions of a member do not overlap one another, and no insertion lies inside a
    deletion (so none lies inside a deletion that a boundary splits).  Then
      (a) the applied slices, concatenated, are the applied whole;
      (b) node_end - node_start of every slice is the length of its applied sequence, and the coordinates of consecutive slices meet."""
    rng = np.random.default_rng(1000 + seed)
    L = int(rng.integers(30, 400))
    n_int = int(rng.integers(1, min(L // 3, 40)))
    b = sc.random_block(rng, L, 12, int(rng.integers(0, L // 6)), n_int, shuffled=seed % 2 == 1, specials=False)
    ivs = b["intervals"]
    assert ivs[0]["start"] == 0 and ivs[-1]["end"] == L and all(a["end"] == c["start"] for a, c in zip(ivs, ivs[1:]))
    for ed in b["members"]:
        spans = sorted((p, p + n) for p, n in ed["dels"] if n)
        assert all(a[1] <= c[0] for a, c in zip(spans, spans[1:]))
        assert not any(p < q < p + n for p, n in ed["dels"] for q, _ in ed["inss"])
        whole = sr.apply(ed, b["consensus"])
        parts, at = [], 0
        for i in ivs:
            part = sr.apply(sr.slice_edits(i, ed, L), b["consensus"][i["start"]:i["end"]])
            s, e = sr.interval_node_coords(i, ed, L)
            assert e - s == len(part) and s == at
            at = e
            parts.append(part)
        assert "".join(parts) == whole and at == len(whole)


def test_slice_structs_match_the_header(tmp_path):
    from pangraph_amd import slice as sl
    pairs = [("pga_slice_block_t", sl.slice_block_t), ("pga_slice_interval_t", sl.slice_interval_t), ("pga_slice_node_t", sl.slice_node_t),
             ("pga_slice_member_t", sl.slice_member_t), ("pga_slice_res_t", sl.slice_res_t), ("pga_slice_out_t", sl.slice_out_t)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {']
    exp = []
    for name, ct in pairs:
        lines.append(f'  printf("%zu", sizeof({name}));')
        lines += [f'  printf(" %zu", offsetof({name}, {f[0]}));' for f in ct._fields_]
        lines.append('  printf("\\n");')
        exp.append([str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_])
    lines += ['  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    assert got == exp
