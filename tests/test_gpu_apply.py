"""pga_apply_merge (pga_apply.hip: the graph update of a merge round on the device) and reweave(update="device") against the host reweave() of
pangraph_amd/reweave.py (through tests/apply_gen.py: host_apply).  Every comparison is exact."""
import ctypes as C
import json
import os

import pytest

import apply_gen as ag
import reweave_gen as rg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import apply as ap  # noqa: E402
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import reweave as rw  # noqa: E402
from pangraph_amd import simplify as sp  # noqa: E402
from pangraph_amd import topology as tp  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))


def check(dll, c):
    got = ap.apply_merge(*c["args"], dll=dll)
    for f in ag.OUT_FIELDS:
        assert got[f] == c["exp"][f], (f, got[f] if len(str(got[f])) < 2000 else "...", c["exp"][f] if len(str(c["exp"][f])) < 2000 else "...")
    return got


# ---------------------------------------------------------------- 1. the named cases and seeded random graphs
@pytest.mark.parametrize("name", sorted(ag.CASES))
def test_named_case(gpu_lib, name):
    check(gpu_lib.dll, ag.case(name))


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_graphs(gpu_lib, seeds):
    for seed in seeds:
        check(gpu_lib.dll, ag.random_case(seed))


# ---------------------------------------------------------------- 2. reweave with the three device calls
def test_reweave_with_the_update_on_the_device(gpu_lib):
    g0, matches = rg.reference_graph(VEC)
    g1, _ = rg.reference_graph(VEC)
    thr = VEC["reweave"]["thr_len"]
    want_g, want_p = rw.reweave(g0, matches, thr, dll=gpu_lib.dll)
    got_g, got_p = rw.reweave(g1, matches, thr, dll=gpu_lib.dll, update="device")
    assert got_g == want_g and got_p == want_p and len(got_p) == 4
    assert want_g["nodes"] == ag.case("reference")["after"]["nodes"] and want_g["paths"] == ag.case("reference")["after"]["paths"]
    for seed in range(4):
        g, ms = ag.random_graph(seed)
        want = rw.reweave(ag.random_graph(seed)[0], ms, rg.THR, dll=gpu_lib.dll)
        assert rw.reweave(g, ms, rg.THR, dll=gpu_lib.dll, update="device") == want


# ---------------------------------------------------------------- 3. a call's graph is the next call's input, by pointer
def _raw(dll, c, graph_args=None):
    K = ap.pack_cut_lists(*c["args"][3:])
    args = graph_args or tp.pack_lists(*c["args"][:3])
    return ap.apply_merge_raw(args, *K, dll=dll, keep=(args, K))


def test_two_rounds_chained_by_pointer(gpu_lib):
    n_second = 0
    for k, c in enumerate([ag.case("reference"), ag.case("forty_intervals"), ag.case("interleaved_merge")] + [ag.random_case(seed) for seed in range(10)]):
        nxt = ag.fresh_cut(c, k)
        if nxt is None or not nxt["args"][3]:
            continue
        first = _raw(gpu_lib.dll, c)
        try:
            assert tp.unpack_lists(first.graph_args()) == nxt["args"][:3]
            second = _raw(gpu_lib.dll, nxt, first.graph_args())
            try:
                got = second.to_lists(len(nxt["args"][0]))
                for f in ag.OUT_FIELDS:
                    assert got[f] == nxt["exp"][f], (f, got[f], nxt["exp"][f])
                n_second += 1
            finally:
                second.free()
        finally:
            first.free()
    assert n_second >= 8


def test_output_graph_is_the_input_of_plan_simplify(gpu_lib):
    n_edges = 0
    for c in ag.simplify_cases():
        after = c["after"]
        index = {b[0]: i for i, b in enumerate(c["exp"]["blocks"])}
        want = [(index[e[0][0]], index[e[1][0]], "+-".index(e[0][1]), "+-".index(e[1][1]), len(after["blocks"][e[0][0]]["alignments"])) for e in sp.find_transitive_edges(after)]
        out = _raw(gpu_lib.dll, c)
        try:
            plan = tp.plan_round_raw(out.graph_args(), flags=tp.EDGES_ONLY, dll=gpu_lib.dll)
            try:
                assert plan.transitive() == want and plan.n_round == 0
            finally:
                plan.free()
        finally:
            out.free()
        n_edges += len(want)
    assert n_edges >= 50                                                       # (tests/test_apply_cpu.py holds the cases to that)


# ---------------------------------------------------------------- 4. malformed input
def test_malformed_input_fails_the_call_and_leaves_the_output_zeroed(gpu_lib):
    dll = gpu_lib.dll
    good = ag.case("two_nodes_one_block")                                       # path 1 (circular): A+ A- B+; A (index 0) in two unaligned intervals
    blocks, paths, nodes, cut, ivs, slices, members = good["args"]
    assert len(blocks) == 2 and cut == [(0, 2, 0)] and slices == [(0, 2, 0), (2, 2, 0)] and members[0][0] == 0 and members[1][0] == 1
    ap._bind(dll)
    check(dll, good)

    def fails(needle, blocks=blocks, paths=paths, nodes=nodes, cut=cut, ivs=ivs, slices=slices, members=members, counts=None):
        args = list(tp.pack_lists(blocks, paths, nodes))
        for at, n in (counts or {}).items():
            args[at] = n
        K = ap.pack_cut_lists(cut, ivs, slices, members)
        out = ap.apply_out_t()
        C.memset(C.byref(out), 0xAB, C.sizeof(out))
        assert dll.pga_apply_merge(*args, K[0], *[C.cast(x, C.c_void_p) for x in K[1:]], C.byref(out)) == -1
        msg = dll.pga_last_error().decode()
        assert msg.startswith("pga_apply_merge: ") and needle in msg, msg
        assert bytes(out) == bytes(C.sizeof(out))
        with pytest.raises(batch.PgaError, match="pga_apply_merge"):
            ap.apply_merge(blocks, paths, nodes, cut, ivs, slices, members, dll=dll) if not counts else ap.apply_merge_raw(args, *K, dll=dll)
        check(dll, good)                                                        # the next call works

    edit = lambda rows, i, **kw: [tuple(kw.get(f, v) for f, v in zip(kw["_f"], r)) if k == i else r for k, r in enumerate(rows)]
    iv = lambda i, **kw: [dict(x, **kw) if k == i else x for k, x in enumerate(ivs)]
    B, P, N = ("id", "len", "depth", "alive"), ("id", "off", "n", "circular"), ("id", "pos0", "pos1", "block", "member", "reverse")
    # what pga_plan_simplify refuses about the graph
    fails("strictly ascending", blocks=edit(blocks, 1, _f=B, id=blocks[0][0]))
    fails("path ids", paths=paths + [(paths[0][0], 3, 0, 0)])
    fails("out of range", nodes=edit(nodes, 2, _f=N, block=2))
    fails("dead block", blocks=edit(blocks, 1, _f=B, alive=0))
    fails("member >= depth", nodes=edit(nodes, 2, _f=N, member=1))
    fails("do not sum", paths=edit(paths, 0, _f=P, n=2))
    fails("running sum", paths=edit(paths, 0, _f=P, off=1))
    for at in (0, 2, 4):
        fails("2^31", counts={at: 1 << 31})
    fails("sum to", blocks=edit(blocks, 1, _f=B, depth=2))
    # the cut
    fails("out of range", cut=[(2, 2, 0)])
    fails("dead", blocks=blocks + [(99, 0, 0, 0)], cut=[(2, 2, 0)])
    fails("named twice", cut=[(0, 1, 0), (0, 1, 1)])
    fails("without intervals", cut=[(0, 0, 0)])
    fails("running sum of n_intervals", cut=[(0, 2, 1)])
    fails("ascending and disjoint", ivs=iv(1, start=ivs[0]["end"] - 1))
    fails("ascending and disjoint", ivs=iv(0, end=ivs[0]["start"]))
    fails("without its partner", ivs=iv(0, aligned=1, is_anchor=1))
    fails("without its partner", ivs=[dict(x, aligned=1, is_anchor=1, new_block_id=77) for x in ivs])      # two anchors of one id
    fails("do not match members", slices=[(0, 3, 0), (3, 1, 0)])
    fails("do not match members", slices=[(0, 2, 0), (3, 2, 0)])
    # found on the device, before any index derived from it is used
    fails("member >= depth", members=edit(members, 0, _f=("m", "r", "a", "b"), m=7))
    fails("kept twice", members=edit(members, 1, _f=("m", "r", "a", "b"), m=0))
    fails("equals a surviving", ivs=iv(0, new_block_id=blocks[1][0]))
    fails("same id", ivs=iv(1, new_block_id=ivs[0]["new_block_id"]))
    fails("equal node ids", members=[members[0], (1,) + members[0][1:]] + members[2:])
    fails("named by", nodes=edit(nodes, 1, _f=N, member=0))
    # an empty cut: no device call, nothing comes back
    got = ap.apply_merge(blocks, paths, nodes, [], [], [], [], dll=dll)
    assert got == {f: None if f in ("blocks", "paths", "nodes") else [] for f in ag.OUT_FIELDS}
    check(dll, good)
