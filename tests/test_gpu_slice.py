"""pga_slice_blocks (block_slice, slice.rs:12-202, on the device for every interval of every block of a merge) against the restatement
tests/slice_ref.py.  Every comparison covers all outputs: the slice records, every field of the kept members (offsets included), the dropped
members and the three edit arrays (tests/slice_cases.py: assert_same)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import slice_cases as sc
import slice_ref as sr
from conftest import GOLDEN
from slice_cases import E

pytestmark = pytest.mark.gpu

V = json.load(open(os.path.join(GOLDEN, "slice_vectors.json")))
WAVE = 64            # edits one wave of k_slice_write / k_slice_count places per step, members one wave of k_slice_scan_local ranks per step,
#                      slices the one wave of k_slice_scan_slices sums per step (pga_slice.hip): 63 / 64 / 65 straddle each of them


def _run(gpu_lib, blocks):
    from pangraph_amd.slice import slice_blocks
    return slice_blocks(sc.for_product(blocks), dll=gpu_lib.dll)


def test_reference_vectors_through_the_product(gpu_lib):
    blocks = sc.vector_blocks(V)
    got = _run(gpu_lib, blocks)
    sc.assert_same(got, sc.expected(blocks))
    # and against the recorded values themselves, not only the restatement
    ex = V["example"]
    for g, s in zip(got[0], ex["slices"]):
        k = g["kept"][0]
        assert (k["subs"], k["dels"], k["inss"], k["node"]) == ([tuple(x) for x in s["subs"]], [tuple(x) for x in s["dels"]], [tuple(x) for x in s["inss"]], tuple(s["node_coords"]))
    assert got[1][0]["kept"][0]["node"] == tuple(V["node_coords"]["expected"])
    for rows, case in zip(got[2:4], V["block_slice"]["cases"]):
        assert rows[0]["dropped"] == []
        for k, n, e in zip(rows[0]["kept"], case["nodes"], case["edits"]):
            assert (k["reverse"], k["pos"]) == (n["reverse"], tuple(n["position"]))
            assert {f: k[f] for f in ("subs", "dels", "inss")} == sc.edit_from_json(e)
    for rows, c in zip(got[4:], V["new_position_circular"] + V["new_position_non_circular"]):
        assert rows[0]["kept"][0]["pos"] == tuple(c["expected"])


def _edge_blocks():
    rng = np.random.default_rng(11)
    L = 100
    cons = sc.random_seq(rng, L)
    I = sr.interval
    tiles = [I(0, 20), I(20, 40, True, True, True), I(40, 60, True, False, True), I(60, 80, True, False, False), I(80, 100)]   # flip only on the third
    early = [I(5, 20), I(20, 40, True, False, True), I(45, 60), I(60, 90)]                                                    # gaps, and the last one ends before the block
    lin = (500, 700, 10000, False, False)
    members = [
        E(subs=[(20, "A"), (39, "C"), (40, "G"), (0, "T"), (99, "A")], dels=[(20, 1), (39, 1), (40, 2)], inss=[(20, "A"), (39, "CC"), (40, "G"), (0, "T")]),   # at start, end - 1, end
        E(dels=[(30, 0), (20, 0), (40, 0), (99, 0), (100, 0)]),                                           # zero length: inside, at a start, at the very end
        E(dels=[(10, 60)]), E(dels=[(0, 100)]), E(dels=[(19, 2), (39, 42)]),                              # over three and more intervals, the whole block
        E(inss=[(100, "ACGT"), (100, "T")]), E(inss=[(100, "A"), (99, "C"), (80, "G")], dels=[(90, 10)]),  # at cons_len
        E(subs=[(70, "A"), (5, "C"), (45, "G"), (21, "T"), (5, "A")], dels=[(85, 3), (3, 4), (50, 20), (22, 1)], inss=[(61, "AA"), (7, "C"), (61, "G"), (33, "T")]),   # unsorted; two at one position
        E(subs=[(25, "A"), (25, "C")], dels=[(27, 2), (27, 3)], inss=[(30, "AC"), (30, "A")]),            # two edits at one position
        E(dels=[(20, 20)]), E(dels=[(20, 10), (30, 10)]), E(dels=[(15, 30)], inss=[(40, "A")]),           # deleted whole in one slice, alive in the next
        E(dels=[(20, 12), (24, 8)]), E(dels=[(24, 8), (20, 12)]),                                         # lengths add up to the slice [20, 40), [32, 40) stays: kept
        E(dels=[(20, 12), (28, 12)]),                                                                     # overlapping and covering: dropped
        E(dels=[(20, 20)], inss=[(25, "")]), E(dels=[(20, 20)], inss=[(25, "A")]),                        # an insertion without letters does not keep a member
        E(),
    ]
    nodes = [lin] * len(members)
    blocks = [dict(consensus=cons, members=members, nodes=nodes, intervals=tiles),
              dict(consensus=cons, members=members, nodes=nodes, intervals=early),
              dict(consensus=cons, members=[], nodes=[], intervals=tiles),                                # a block with no members
              dict(consensus=cons, members=[E(), E(subs=[(3, "A")])], nodes=[lin, lin], intervals=[]),   # ... and one that is not cut at all
              dict(consensus=cons, members=[E()], nodes=[lin], intervals=[I(0, 100)])]
    # nodes: circular ones that wrap ((95, 20) of 100) or span their whole path, reverse ones, linear reverse; flip on and off
    few = [E(), E(dels=[(10, 5)], inss=[(50, "ACG")]), E(inss=[(0, "AC"), (100, "G")], dels=[(95, 5)])]
    for node in [(95, 20, 100, False, True), (95, 20, 100, True, True), (0, 100, 100, False, True), (0, 0, 100, True, True), (7, 7, 125, False, True),
                 (1000, 1125, 5000, True, False), (0, 125, 125, False, False), (0, 125, 125, True, False)]:
        blocks.append(dict(consensus=cons, members=few, nodes=[node] * len(few), intervals=tiles))
    return blocks


def test_edge_shapes(gpu_lib):
    blocks = _edge_blocks()
    exp = sc.expected(blocks)
    sc.assert_same(_run(gpu_lib, blocks), exp)
    tiles = exp[0]
    assert 9 in tiles[1]["dropped"] and 9 not in tiles[2]["dropped"]                                     # deleted whole in [20, 40), alive in [40, 60)
    assert {12, 13} <= {k["member"] for k in tiles[1]["kept"]} and 14 in tiles[1]["dropped"]
    assert 15 in tiles[1]["dropped"] and 16 not in tiles[1]["dropped"]
    assert exp[2] == [dict(member_off=r["member_off"], kept=[], dropped=[]) for r in exp[2]] and exp[3] == []
    assert any(k["reverse"] != bool(n[3]) for b, rows in zip(blocks[5:], exp[5:]) for r in rows for k, n in zip(r["kept"], b["nodes"]))   # a flipped strand


# ---- random blocks: built once, shared by the tests below, never modified ----
def _random_blocks():
    rng = np.random.default_rng(2026)
    blocks = []
    # every list length with every interval count, sorted and shuffled; every member count where the block is cut a few times (the deep blocks
    # cut many times would only make the restatement slow: its cost is intervals x members x edits)
    lens, ints, mems = (0, 1, WAVE - 1, WAVE, WAVE + 1, 200), (1, 2, WAVE, WAVE + 1, 300), (1, 3, WAVE, WAVE + 1, 130)
    k = 0
    for n_list in lens:
        for n_int in ints:
            n_mem = (1, 3)[k % 2] if n_int > 2 or n_list > WAVE + 1 else mems[k % len(mems)]
            L = int(rng.integers(max(3 * n_int, 2 * n_list + 40), 4097)) if n_int > 2 or n_list > 1 else int(rng.integers(8, 300))
            blocks.append(sc.random_block(rng, L, n_mem, n_list, n_int, shuffled=k % 2 == 1, gaps=k % 5 == 4))
            k += 1
    # every member count once more on short lists, deep blocks cut WAVE + 1 and 300 times, and one deep block of long lists
    for n_mem in mems:
        blocks.append(sc.random_block(rng, 1500, n_mem, 7, 9, shuffled=n_mem % 2 == 1))
    blocks.append(sc.random_block(rng, 2000, WAVE + 1, 2, WAVE + 1, gaps=True))
    blocks.append(sc.random_block(rng, 4096, 10, 5, 300, shuffled=True))
    blocks.append(sc.random_block(rng, 4096, WAVE + 1, 200, 5, shuffled=True))
    return blocks


@pytest.fixture(scope="module")
def random_blocks():
    blocks = _random_blocks()
    return blocks, sc.expected(blocks)


def test_random_blocks_vs_restatement(gpu_lib, random_blocks):
    blocks, exp = random_blocks
    sc.assert_same(_run(gpu_lib, blocks), exp)


def test_random_blocks_exercise_what_they_are_for(random_blocks):
    """the generated inputs hold what the comparison above is there for: a dropped member, a deletion over more than two intervals, an
    insertion at the end of the block that is sliced, and an emptiness candidate that is kept"""
    blocks, exp = random_blocks
    assert sum(len(r["dropped"]) for rows in exp for r in rows) > 0
    n_wide = n_end = n_candidate_kept = 0
    for b, rows in zip(blocks, exp):
        L, ivs = len(b["consensus"]), b["intervals"]
        for e in b["members"]:
            n_wide += sum(1 for p, n in e["dels"] if sum(1 for i in ivs if sr.has_overlap_with(i, p, p + n)) > 2)
            n_end += sum(1 for p, _ in e["inss"] if p == L and ivs[-1]["end"] == L)
        for i, r in zip(ivs, rows):
            n_candidate_kept += sum(1 for k in r["kept"] if not sum(len(s) for _, s in k["inss"]) and sum(n for _, n in k["dels"]) >= i["end"] - i["start"])
    assert n_wide > 0 and n_end > 0 and n_candidate_kept > 0
    assert {len(b["members"]) for b in blocks} >= {1, 3, 64, 65, 130} and {len(b["intervals"]) for b in blocks} >= {1, 2, 64, 65, 300}
    assert {len(e["dels"]) for b in blocks for e in b["members"]} >= {0, 1, 63, 64, 65, 200}


def test_hand_over_to_the_promise_entry(gpu_lib):
    """the kept members of an aligned slice go to pga_stage_promise_jobs as they come out: counts + member_off, the three edit arrays at the
    first kept member's offsets, the caller's ins_seq, the consensus at consensus + start -- pointer arithmetic only.  With a <len>M CIGAR
    onto the same consensus it builds every member's sequence: apply(sliced edits, sliced consensus) of the restatement."""
    from pangraph_amd.promise import pack_cigar, promise_t
    from pangraph_amd.slice import slice_blocks_raw
    from pangraph_amd.mapvar import del_t, ins_t, sub_t
    from pangraph_amd.reconsensus import rc_member_t
    rng = np.random.default_rng(4)
    blocks = [sc.random_block(rng, 600, 9, 12, 4), sc.random_block(rng, 300, 5, 6, 3, shuffled=True)]
    exp = sc.expected(blocks)
    K, out, free = slice_blocks_raw(sc.for_product(blocks), dll=gpu_lib.dll)
    dll = gpu_lib.dll
    dll.pga_stage_promise_jobs.restype = C.c_int
    dll.pga_stage_promise_jobs.argtypes = [C.c_int64] + [C.c_void_p] * 10 + [C.POINTER(C.POINTER(C.c_char))]
    dll.pga_free.argtypes = [C.c_void_p]
    try:
        s = n_checked = 0
        for bi, (b, rows) in enumerate(zip(blocks, exp)):
            cons_at = C.cast(C.c_char_p(K.cons[bi]), C.c_void_p).value          # the buffer pga_slice_block_t.consensus points to
            for i, r in zip(b["intervals"], rows):
                res = out.slices[s]
                s += 1
                if res.n_kept == 0:
                    continue
                first = out.members[res.member_off]
                ln = i["end"] - i["start"]
                words = (C.c_uint32 * 1)(*pack_cigar([(ln, "M")]))
                P = promise_t()
                P.anchor = P.append = cons_at + i["start"]
                P.anchor_len = P.append_len = ln
                P.reverse = 0; P.cigar = C.cast(words, C.POINTER(C.c_uint32)); P.n_cigar = 1; P.n_members = res.n_kept
                n = res.n_kept
                status = (C.c_int32 * n)(); ms = (C.c_int32 * n)(); bw = (C.c_uint32 * n)(); off = (C.c_uint64 * (n + 1))()
                seqs = C.POINTER(C.c_char)()
                rc = dll.pga_stage_promise_jobs(1, C.byref(P), C.addressof(out.counts.contents) + res.member_off * C.sizeof(rc_member_t),
                                                C.addressof(out.subs.contents) + first.sub_off * C.sizeof(sub_t), C.addressof(out.dels.contents) + first.del_off * C.sizeof(del_t),
                                                C.addressof(out.inss.contents) + first.ins_off * C.sizeof(ins_t), K.L, status, ms, bw, off, C.byref(seqs))
                assert rc == 0, dll.pga_last_error()
                try:
                    base = C.addressof(seqs.contents)
                    sliced = b["consensus"][i["start"]:i["end"]]
                    for t, k in enumerate(r["kept"]):
                        want = sr.apply(k, sliced)
                        assert want and status[t] in (0, 7)                 # (7: no aligned position left -- the sequence is built all the same, but not handed out)
                        if status[t] == 0:
                            assert C.string_at(base + off[t], off[t + 1] - off[t]).decode() == want
                            n_checked += 1
                finally:
                    dll.pga_free(C.cast(seqs, C.c_void_p))
        assert n_checked >= 30
    finally:
        free()


def test_malformed_input_fails_the_call(gpu_lib):
    from pangraph_amd.batch import PgaError
    from pangraph_amd.slice import _Packed, _bind, slice_blocks, slice_out_t
    cons = "ACGTACGTAC" * 3
    lin = (0, 30, 100, False, False)
    ok = dict(consensus=cons, members=[E(dels=[(3, 4)])], nodes=[lin], intervals=[(0, 10, 0), (10, 30, 1)])

    def bad(match, **kw):
        with pytest.raises(PgaError, match=match):
            slice_blocks([ok, dict(ok, **kw)], dll=gpu_lib.dll)
        assert len(slice_blocks([ok], dll=gpu_lib.dll)[0]) == 2                 # a valid call right after succeeds

    for ivs in ([(10, 30, 0), (0, 10, 0)], [(0, 12, 0), (10, 30, 0)], [(5, 5, 0)], [(7, 5, 0)], [(0, 31, 0)]):
        bad("intervals of block 1", intervals=ivs)
    bad("substitution beyond the consensus", members=[E(subs=[(30, "A")])])
    bad("deletion beyond the consensus", members=[E(dels=[(25, 6)])])
    bad("insertion beyond the consensus", members=[E(inss=[(31, "A")])])
    bad("empty consensus", consensus="", members=[E()], intervals=[])
    bad("path of length 0", nodes=[(0, 0, 0, False, True)])
    bad("pos_end < node_end", nodes=[(0, 20, 100, True, False)])                # the second slice has node_end = 26
    bad("overlapping deletions", members=[E(dels=[(0, 6), (0, 6)])])            # twelve positions counted before the boundary at 10
    # a NULL list with a non-zero count
    dll = gpu_lib.dll
    _bind(dll)
    K = _Packed([ok])
    out = slice_out_t()
    for hole in (2, 3, 4, 6):                                                   # intervals, members, nodes, deletions
        args = list(K.args())
        args[hole] = None
        assert dll.pga_slice_blocks(*args, C.byref(out)) == -1 and b"null" in dll.pga_last_error()
    assert dll.pga_slice_blocks(*K.args(), None) == -1
    assert dll.pga_slice_blocks(*K.args(), C.byref(out)) == 0 and out.slices[1].n_kept == 1
    dll.pga_slice_free(C.byref(out))
    assert slice_blocks([], dll=gpu_lib.dll) == []
