"""SURVEY 8(f)-1, the whole step: pga_solve_promises / pga_stage_promise_jobs (MergePromise::solve_promise, reweave.rs:40-94, on the device)
against the restatement tests/promise_ref.py over the oracle's map_variations (oracle/pgo_mapvar.c)."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import mapvarbind as mb
import promise_ref as pr
from conftest import ROOT

pytestmark = pytest.mark.gpu

TILE = 1024          # letters one workgroup of k_promise_build writes (256 threads x 4 letters, pga_promise.hip)


def E(inss=(), dels=(), subs=()):
    return {"inss": list(inss), "dels": list(dels), "subs": list(subs)}


def _both_ways(anchor, append, cigar, members):
    ops = pr.parse_cigar(cigar) if isinstance(cigar, str) else cigar
    return [(anchor, append, False, ops, members), (anchor, append, True, ops, members)]


def test_stage_jobs_on_edge_shapes(gpu_lib):
    from pangraph_amd.promise import stage_jobs
    rng = np.random.default_rng(5)
    L = TILE + 80
    cons = mb.random_seq(rng, L)
    promises = []
    # built lengths around a wave, around the kernel's tile, and none at all: the first n letters, the last n, and n letters from both ends
    members = []
    for n in (0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1):
        members += [E(dels=[(n, L - n)]), E(dels=[(0, L - n)])]
        if n >= 2:
            members.append(E(dels=[(n // 2, L - n)]))
    members.append(E())
    promises += _both_ways(cons, cons, f"{L}M", members)
    # the same lengths reached with insertions, so that a tile holds runs of all three kinds
    short = mb.random_seq(rng, 40)
    members = [E(inss=[(20, mb.random_seq(rng, n - 40))], subs=[(3, "A"), (39, "C")]) for n in (63, 64, 65, TILE - 1, TILE, TILE + 1)]
    promises += _both_ways(short, short, "40M", members)
    c100 = mb.random_seq(rng, 100)
    big = mb.random_seq(rng, 5000)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    members = [
        E(inss=[(0, "ACGGT")]), E(inss=[(100, "TTGCA")]), E(inss=[(0, "AC"), (100, "GT")]),
        E(inss=[(5, "TT"), (5, "AC")]), E(inss=[(5, "AC"), (5, "A"), (5, "ACG")]),                 # one position: ordered by letters
        E(inss=[(50, big)]), E(inss=[(0, big)], dels=[(0, 100)]),
        E(dels=[(0, 3)]), E(dels=[(97, 3)]), E(dels=[(0, 3), (97, 3)]),
        E(dels=[(10, 5), (15, 5)]), E(dels=[(15, 5), (10, 5)]), E(dels=[(10, 10), (15, 10)]), E(dels=[(10, 0), (10, 4)]),
        E(dels=[(10, 5)], subs=[(12, other[c100[12]])]),                                          # a substitution inside a deletion
        E(subs=[(7, other[c100[7]]), (7, other[other[c100[7]]])]),                                # two at one position: the last wins
        E(subs=[(99, other[c100[99]]), (0, other[c100[0]]), (50, other[c100[50]])]),              # not in order
        E(dels=[(10, 10)], inss=[(15, "ACG")]), E(dels=[(10, 10)], inss=[(10, "AC"), (20, "GT")]),  # insertions inside and at the ends of a deletion
        E(inss=[(30, "YKM"), (60, "RWSN")], subs=[(1, "R"), (2, "B")]),
        E(dels=[(0, 100)]), E(dels=[(0, 100)], inss=[(40, "ACGT")]),
    ]
    promises += _both_ways(c100, c100, "100M", members)
    iupac = "ACGTYRWSKMDVHBN" * 5
    promises += _both_ways(iupac, iupac, f"{len(iupac)}M", [E(), E(dels=[(3, 7)], inss=[(20, "HDVB")], subs=[(0, "N")])])
    # letters the complement rejects: in the consensus (seen only by the kernel), in an insertion, in a substitution a deletion hides, lower case
    bad = c100[:40] + "X" + c100[41:]
    promises += _both_ways(c100, bad, "100M", [E(), E(dels=[(40, 1)]), E(subs=[(40, "A")])])
    promises += _both_ways(c100, c100, "100M", [E(inss=[(9, "AXA")]), E(dels=[(10, 5)], subs=[(12, "X")]), E(subs=[(12, "a")]), E(dels=[(0, 100)], inss=[(4, "AXA")])])
    # the promises of reweave.rs::test_reweave, and one with = and X
    for cigar in ("200M", "10I20D170M10I10M", "100M50D", "80M10I10M10D", "50=2X48="):
        ops = pr.parse_cigar(cigar)
        ref_len = sum(n for n, op in ops if op in "M=XD")
        qry_len = sum(n for n, op in ops if op in "M=XI")
        app = mb.random_seq(rng, qry_len)
        promises += _both_ways(mb.random_seq(rng, ref_len), app, ops, [E(), E(dels=[(5, 10)], inss=[(40, "ACGTA")]), E(inss=[(0, "AC")], dels=[(qry_len - 4, 4)])])
    got = stage_jobs(promises, dll=gpu_lib.dll)
    seen = set()
    for q, g in zip(promises, got):
        exp = pr.stage_promise(q)
        assert g == exp, (q[2], q[3], [i for i, (a, b) in enumerate(zip(g, exp)) if a != b][:4])
        seen |= set(e[0] for e in exp)
    assert seen == {0, 7, 9}


# ---- random promises: built once, shared by the tests below, never modified ----
def _random_promise(rng, oracle_dll, L, depth, reverse, band=60, **rates):
    anchor = mb.random_seq(rng, L)
    oriented = mb.mutate(rng, anchor, **rates) or "A"                                   # what the aligner saw of the append consensus
    append = pr.reverse_complement(oriented) if reverse else oriented
    a = mb.oracle_map_variations(oracle_dll, anchor, oriented, 0, band, want_aln=True)
    assert a["status"] == 0
    cigar = pr.cigar_from_alignment(a["ref_aln"], a["qry_aln"])
    members = []
    for _ in range(depth):
        seq = mb.mutate(rng, append, **rates) or "A"
        g = mb.oracle_map_variations(oracle_dll, append, seq, 0, band)
        assert g["status"] == 0
        e = E(g["inss"], g["dels"], g["subs"])
        assert mb.apply_edit(append, e) == seq
        members.append(e)
    return (anchor, append, reverse, cigar, members)


@pytest.fixture(scope="module")
def random_promises(oracle_lib):
    rng = np.random.default_rng(77)
    promises = []
    for i in range(24):
        if i == 12:                                                                     # one deep block of long members, in the middle
            promises.append(_random_promise(rng, oracle_lib.dll, 20000, 64, True, band=30, snp=0.01, indel=0.001, max_indel=10))
        promises.append(_random_promise(rng, oracle_lib.dll, int(rng.integers(50, 3001)), int(rng.integers(1, 13)), i % 2 == 1))
    restated = [pr.stage_promise(q) for q in promises]
    expected = [pr.solve_promise(oracle_lib.dll, q) for q in promises]
    return promises, restated, expected


def test_random_promises_vs_restatement(gpu_lib, random_promises):
    from pangraph_amd.promise import solve_promises
    promises, restated, expected = random_promises
    got = solve_promises(promises, dll=gpu_lib.dll)
    n = 0
    for q, g, exp in zip(promises, got, expected):
        assert len(g) == len(exp)
        for a, b in zip(g, exp):
            assert a == b
            assert a["status"] == 0
            n += 1
    assert n >= 24 + 64
    # and the members are still the same sequences, now spelled against the anchor consensus
    for q, g, st in zip(promises, got, restated):
        for a, s in zip(g, st):
            assert mb.apply_edit(q[0], a) == s[3]


def test_same_answer_as_map_variations_on_host_built_sequences(gpu_lib, random_promises):
    from pangraph_amd.promise import solve_promises
    promises, restated, _ = random_promises
    jobs = [(q[0], s[3], s[1], s[2]) for q, st in zip(promises, restated) for s in st]
    assert all(s[0] == 0 and s[3] for st in restated for s in st)
    via_sequences = mb.product_map_variations(gpu_lib.dll, jobs)
    got = [a for g in solve_promises(promises, dll=gpu_lib.dll) for a in g]
    assert got == via_sequences


def _raw_bytes(promises, dll=None):
    from pangraph_amd.promise import del_t, ins_t, solve_promises_raw, sub_t
    K, R, subs, dels, inss, iseq, free = solve_promises_raw(promises, dll=dll)
    try:
        n = K.n_mem
        tot = [sum(getattr(R[m], f) for m in range(n)) for f in ("n_subs", "n_dels", "n_inss", "n_ins_bases")]
        return [C.string_at(C.addressof(R), n * C.sizeof(R[0])), C.string_at(subs, tot[0] * C.sizeof(sub_t)), C.string_at(dels, tot[1] * C.sizeof(del_t)),
                C.string_at(inss, tot[2] * C.sizeof(ins_t)), C.string_at(iseq, tot[3])]
    finally:
        free()


def test_chunked_run_equals_one_chunk(gpu_lib, random_promises, tmp_path):
    promises = random_promises[0]
    whole = _raw_bytes(promises, gpu_lib.dll)
    assert len(whole[0]) == 56 * sum(len(q[4]) for q in promises) and len(whole[1]) > 0 and len(whole[4]) > 0
    src, dst = tmp_path / "promises.pkl", tmp_path / "bytes.pkl"
    src.write_bytes(pickle.dumps(promises))
    code = ("import pickle, sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']; import test_gpu_promise as t; "
            "pickle.dump(t._raw_bytes(pickle.load(open(sys.argv[2], 'rb'))), open(sys.argv[3], 'wb'))")
    env = dict(os.environ, PGA_PROMISE_CHUNK_MB="1")                                     # the deep block alone is larger: at least three chunks
    r = subprocess.run([sys.executable, "-c", code, ROOT, str(src), str(dst)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert pickle.loads(dst.read_bytes()) == whole


def test_statuses_and_rejected_calls(gpu_lib):
    from pangraph_amd.batch import PgaError
    from pangraph_amd.promise import solve_promises
    rng = np.random.default_rng(3)
    anchor = mb.random_seq(rng, 60)
    append = anchor[:50]
    none, whole, plus = E(), E(dels=[(0, 50)]), E(dels=[(0, 50)], inss=[(20, "ACGT")])
    alien = E(inss=[(10, "AXA")])
    M50 = [(50, "M"), (10, "D")]
    got = solve_promises([
        (anchor, append, False, [(60, "D")], [none, whole, plus]),                      # no aligned position in the cigar: 8 for all, the empty one too
        (anchor, append, False, M50, [none, whole, plus, alien]),
        (anchor, pr.reverse_complement(append), True, M50, [none, whole, plus, alien]),
        (anchor, append, False, M50, []),                                                # a promise without members
    ], dll=gpu_lib.dll)
    assert [a["status"] for a in got[0]] == [8, 8, 8]
    assert all(a["subs"] == a["dels"] == a["inss"] == [] for a in got[0])
    assert [a["status"] for a in got[1]] == [0, 0, 7, 2]                                 # forward: the aligner's alphabet rejects the X
    assert [a["status"] for a in got[2]] == [0, 0, 7, 9]                                 # reverse: the complement rejects it first
    for g in (got[1], got[2]):
        assert (g[0]["subs"], g[0]["dels"], g[0]["inss"]) == ([], [(50, 10)], [])
        assert (g[1]["subs"], g[1]["dels"], g[1]["inss"], g[1]["score"], g[1]["attempts"]) == ([], [(0, 60)], [], 0, 0)   # Edit::deleted(anchor_len)
    assert got[3] == []
    assert solve_promises([], dll=gpu_lib.dll) == []
    with pytest.raises(PgaError, match="unsupported CIGAR operation 'S'"):
        solve_promises([(anchor, append, False, [(5, "S"), (45, "M")], [none])], dll=gpu_lib.dll)
    with pytest.raises(PgaError, match="deletion beyond the append consensus"):
        solve_promises([(anchor, append, False, M50, [none, E(dels=[(45, 6)])])], dll=gpu_lib.dll)
    with pytest.raises(PgaError, match="substitution beyond the append consensus"):
        solve_promises([(anchor, append, False, M50, [E(subs=[(50, "A")])])], dll=gpu_lib.dll)
    with pytest.raises(PgaError, match="insertion beyond the append consensus"):
        solve_promises([(anchor, append, False, M50, [E(inss=[(51, "A")])])], dll=gpu_lib.dll)
