"""The new pieces of the solve_promise restatement (tests/promise_ref.py) on the reference's own unit-test vectors, recorded as data in
tests/golden/promise_vectors.json: reverse_complement (io/seq.rs:50-65) and Edit::from_cigar (edits.rs:1041-1090); plus the ctypes mirror of
pga_promise_t against the header.  No GPU."""
import ctypes as C
import json
import os
import subprocess

import pytest

import promise_ref as pr
from conftest import GOLDEN, ROOT

V = json.load(open(os.path.join(GOLDEN, "promise_vectors.json")))


@pytest.mark.parametrize("seq,exp", V["reverse_complement"])
def test_reverse_complement(seq, exp):
    assert pr.reverse_complement(seq) == exp


@pytest.mark.parametrize("seq,msg", V["reverse_complement_rejected"])
def test_reverse_complement_rejects(seq, msg):
    with pytest.raises(pr.Rejected) as e:
        pr.reverse_complement(seq)
    assert str(e.value) == msg
    with pytest.raises(pr.Rejected):
        pr.reverse_complement("acgt")                       # lower case is not in the table


@pytest.mark.parametrize("case", V["from_cigar"], ids=lambda c: c["name"])
def test_from_cigar(case):
    e = pr.from_cigar(pr.parse_cigar(case["cigar"]))
    assert e["subs"] == []
    assert e["inss"] == [tuple(x) for x in case["inss"]]
    assert e["dels"] == [tuple(x) for x in case["dels"]]


def test_from_cigar_rejects_other_operations():
    with pytest.raises(NotImplementedError):
        pr.from_cigar(pr.parse_cigar("5S10M"))


def test_edit_reverse_complement_sorts_stably():
    """edits.rs:257-276: positions mirrored (sub len-pos-1, del len-pos-len, ins len-pos), every list sorted by position with ties in the
    mapped order"""
    e = {"subs": [(0, "A"), (9, "C"), (9, "G")], "dels": [(2, 3), (7, 0), (7, 1)], "inss": [(10, "AC"), (4, "T"), (4, "GG"), (0, "R")]}
    r = pr.edit_reverse_complement(e, 10)
    assert r["subs"] == [(0, "G"), (0, "C"), (9, "T")]
    assert r["dels"] == [(2, 1), (3, 0), (5, 3)]
    assert r["inss"] == [(0, "GT"), (6, "A"), (6, "CC"), (10, "Y")]


def test_stage_promise_status_order():
    anchor, append = "ACGTACGTAC", "ACGTACGT"
    whole = {"subs": [], "dels": [(0, 8)], "inss": []}
    plus = {"subs": [], "dels": [(0, 8)], "inss": [(3, "AX")]}
    none = {"subs": [], "dels": [], "inss": []}
    assert pr.stage_promise((anchor, append, False, [(10, "D")], [none, whole])) == [(8, 0, 0, ""), (8, 0, 0, "")]
    assert pr.stage_promise((anchor, append, False, [(8, "M"), (2, "D")], [none, whole, plus])) == [(0, 0, 0, append), (0, 0, 0, ""), (7, 0, 0, "")]
    assert pr.stage_promise((anchor, append, True, [(8, "M"), (2, "D")], [none, whole, plus])) == [(0, 0, 0, "ACGTACGT"), (0, 0, 0, ""), (9, 0, 0, "")]
    # the two bands add up (map_variations.rs:23-26).  By hand: cigar 2M3I6M2D over the anchor of 10 -> 8 aligned positions, total shift
    # -3 * 6 + 2 * 0 = -18, mean round(-2.25) = -2, width max(|0 + 2|, |-3 + 2|) = 2 (the trailing deletion does not count); the member's
    # deletion (1, 2) over the append consensus of 8 -> 6 aligned, total 2 * 5 = 10, mean round(1.67) = 2, width max(|0 - 2|, |2 - 2|) = 2
    e = {"subs": [], "dels": [(1, 2)], "inss": []}
    assert pr.stage_promise((anchor, append, False, pr.parse_cigar("2M3I6M2D"), [e])) == [(0, 0, 4, "ATACGT")]
    # reverse: the deletion becomes (8 - 1 - 2, 2) = (5, 2) -> total 2 * 1 = 2, mean round(0.33) = 0, width max(|0|, |2|) = 2
    assert pr.stage_promise((anchor, append, True, pr.parse_cigar("2M3I6M2D"), [e])) == [(0, -2, 4, "ACGTAT")]


def test_promise_struct_matches_the_header(tmp_path):
    from pangraph_amd import promise
    ct = promise.promise_t
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pga_align.h"', 'int main(void) {', '  printf("%zu", sizeof(pga_promise_t));']
    lines += [f'  printf(" %zu", offsetof(pga_promise_t, {f[0]}));' for f in ct._fields_]
    lines += ['  printf("\\n");', '  return 0;', '}']
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=gnu99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert got == [str(C.sizeof(ct))] + [str(getattr(ct, f[0]).offset) for f in ct._fields_]
    assert promise.pack_cigar([(10, "M"), (3, "="), (2, "X"), (1, "I"), (4, "D")]) == [160, 55, 40, 17, 66]
