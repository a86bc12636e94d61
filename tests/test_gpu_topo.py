"""pga_plan_simplify (pga_topo.hip: the path side of a round of `pangraph simplify` on the device) and simplify(topology="device") against
the host functions of pangraph_amd/simplify.py (through tests/topo_gen.py: host_plan) and the reference's own unit-test values
(tests/golden/simplify_vectors.json).  Every comparison is exact."""
import copy
import gzip
import json
import os

import pytest

import simplify_ref as sr
import topo_gen as tg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import simplify as sp  # noqa: E402
from pangraph_amd import topology as tp  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "simplify_vectors.json")))
MB, CI, SR = VEC["merge_blocks"], VEC["circularize"], VEC["simplify_run"]
FIELDS = ("transitive", "edge_counts", "round", "partner", "new_nodes", "old_left", "old_right", "blocks", "paths", "nodes")


def check(dll, lists, sched=None, flags=tp.COUNTS):
    got = tp.plan_round(*lists, sched=sched, flags=flags, dll=dll)
    exp = tg.host_plan(*lists, sched, flags)
    for f in FIELDS:
        assert got[f] == exp[f], (f, got[f], exp[f])
    return got


def _lists(graph):
    g = sp.normalize(graph)
    return g, tg.to_lists(g, {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()})


def _edge(e, bids):
    return ((bids[e[0]], "+-"[e[2]]), (bids[e[1]], "+-"[e[3]]))


# ---------------------------------------------------------------- 1. the reference's own values
def test_reference_edge_counts_and_transitive_edges(gpu_lib):
    g, lists = _lists(CI["input_graph"])
    bids = [b[0] for b in lists[0]]
    got = check(gpu_lib.dll, lists)
    want = CI["transitive_edges"]
    assert len(got["transitive"]) == len(want) and all(sr.edge_eq(_edge(a, bids), tuple(map(tuple, b))) for a, b in zip(got["transitive"], want))
    counts = [(_edge(e, bids), e[4]) for e in got["edge_counts"]]
    for e, n in CI["edge_counts"]:
        assert [c for k, c in counts if sr.edge_eq(k, tuple(map(tuple, e)))] == [n]
    for e in CI["absent_edges"]:
        assert not [c for k, c in counts if sr.edge_eq(k, tuple(map(tuple, e)))]
    assert len(counts) == len(sr.count_edges(sr.from_json(CI["input_graph"])))
    _, single = _lists(CI["single_block_graph"])
    got = check(gpu_lib.dll, single)
    assert got["transitive"] == [] == CI["single_block_transitive_edges"] and got["round"] == [] and got["nodes"] is None


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_reference_pairings_new_nodes_and_paths(gpu_lib, case):
    v = MB[case]
    g, lists = _lists(v["graph"])
    bids = [b[0] for b in lists[0]]
    got = check(gpu_lib.dll, lists)
    (rnd,) = got["round"]
    assert sr.edge_eq(((bids[rnd["anchor"]], "+-"[rnd["anchor_rev"]]), (bids[rnd["other"]], "+-"[rnd["other_rev"]])), tuple(map(tuple, v["edge"])))
    pairs = dict(zip(got["old_left"], got["old_right"]))
    pairs.update({b: a for a, b in pairs.items()})
    assert pairs == {int(k): n for k, n in MB["pairings"].items()}
    path_of = {n[0]: p[0] for p in got["paths"] for n in got["nodes"][p[1]:p[1] + p[2]]}
    for old, new in list(zip(got["old_left"], got["new_nodes"])) + list(zip(got["old_right"], got["new_nodes"])):
        assert {"block_id": bids[new[3]], "path_id": path_of[new[0]], "strand": "+-"[new[5]], "position": [new[1], new[2]]} == v["new_nodes"][str(old)]
    # the partner list as pga_merge_blocks takes it: slot k of the left block with the slot of its partner in the right block
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    left, right = bids[rnd["merge"][0]], bids[rnd["merge"][1]]
    assert [order[right][q] for q in got["partner"]] == [pairs[n] for n in order[left]]
    # the graph behind the round against expected_graph ('@k' stands for the id of new node k)
    ids = {int(k): sr.node_id(n["block_id"], n["path_id"], n["strand"], n["position"]) for k, n in v["new_nodes"].items()}
    key = lambda k: ids[int(k[1:])] if isinstance(k, str) and k.startswith("@") else int(k)
    exp = v["expected_graph"]
    assert {p[0]: [n[0] for n in got["nodes"][p[1]:p[1] + p[2]]] for p in got["paths"]} == {int(k): [key(n) for n in p["nodes"]] for k, p in exp["paths"].items()}
    assert {n[0]: (bids[n[3]], path_of[n[0]], "+-"[n[5]], (n[1], n[2])) for n in got["nodes"]} == \
        {key(k): (n["block_id"], n["path_id"], n["strand"], tuple(n["position"])) for k, n in exp["nodes"].items()}
    assert [(b[0], b[1]) for b in got["blocks"] if b[3]] == sorted((int(k), len(b["consensus"])) for k, b in exp["blocks"].items())


def test_reference_simplify_run(gpu_lib):
    trace = {}
    got = sp.simplify(SR["graph"], SR["focal"], dll=gpu_lib.dll, topology="device", trace=trace)
    assert got == sr.from_json(SR["expected_graph"]) and set(got["nodes"]) >= {SR["NID11"], SR["NID12"]}
    assert len(trace["rounds"]) == len(trace["transitive"]) >= 1


# ---------------------------------------------------------------- 2. the named cases and seeded random graphs
@pytest.mark.parametrize("name", sorted(tg.CASES))
def test_named_case(gpu_lib, name):
    lists = tg.CASES[name]()
    got = check(gpu_lib.dll, lists)
    edges_only = check(gpu_lib.dll, lists, flags=tp.EDGES_ONLY)
    assert edges_only["transitive"] == got["transitive"] and edges_only["round"] == [] and edges_only["nodes"] is None


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_graphs(gpu_lib, seeds):
    for seed in seeds:
        check(gpu_lib.dll, tg.random_graph(seed))


# ---------------------------------------------------------------- 3. a call's output is the next call's input, by pointer
def test_chained_rounds(gpu_lib):
    n_second = 0
    for lists in [tg.CASES["chain"](), tg.CASES["tile_edges"]()] + [tg.random_graph(seed) for seed in range(12)]:
        nxt = tg.second_round(lists)
        if nxt is None:
            continue
        args = tp.pack_lists(*lists)
        first = tp.plan_round_raw(args, dll=gpu_lib.dll)
        try:
            assert tp.unpack_lists(first.graph_args()) == nxt
            second = tp.plan_round_raw(first.graph_args(), flags=tp.COUNTS, dll=gpu_lib.dll)
            try:
                got, exp = second.to_lists(), tg.host_plan(*nxt, None, tp.COUNTS)
                for f in FIELDS:
                    assert got[f] == exp[f], (f, got[f], exp[f])
                n_second += bool(exp["round"])
            finally:
                second.free()
        finally:
            first.free()
    assert n_second >= 3


# ---------------------------------------------------------------- 4. an explicit round
def test_explicit_round(gpu_lib):
    lists = tg.CASES["chain"]()
    got = check(gpu_lib.dll, lists, sched=[(1, 0, 2, 0)])                       # the middle edge, which the defined round skips
    assert [r["transitive"] for r in got["round"]] == [1]
    assert check(gpu_lib.dll, lists, sched=[(2, 1, 1, 1)])["round"] == got["round"]      # the same edge inverted
    check(gpu_lib.dll, lists, sched=[(2, 0, 3, 0), (0, 0, 1, 0)])               # the order given is the order taken
    four = tg.CASES["four_strands"]()
    t = tg.host_plan(*four)["transitive"]
    check(gpu_lib.dll, four, sched=[(t[3][0], t[3][2], t[3][1], t[3][3]), (t[0][1], 1 - t[0][3], t[0][0], 1 - t[0][2])])


# ---------------------------------------------------------------- 5. the whole command
@pytest.fixture(scope="module")
def plasmids():
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    return G, [G["paths"][k]["name"] for k in sorted(G["paths"], key=int)]


@pytest.mark.parametrize("n_paths", [1, 3, 8])
def test_plasmids_with_the_topology_on_the_device(gpu_lib, plasmids, n_paths):
    G, names = plasmids
    focal = names[:n_paths]
    t0, t1 = {}, {}
    want = sp.simplify(G, focal, dll=gpu_lib.dll, trace=t0)
    got = sp.simplify(G, focal, dll=gpu_lib.dll, trace=t1, topology="device")
    assert got == want and t1["rounds"] == t0["rounds"] and t1["rounds"] and t1["zero_copy"] == t0["zero_copy"]
    assert got == sr.simplify(sr.from_json(G), set(focal), t1["rounds"])        # the golden expectation
    assert all(set(r) <= set(t) for r, t in zip(t1["rounds"], t1["transitive"])) and not sp.find_transitive_edges(got)


def test_a_schedule_through_the_device(gpu_lib):
    (edge,) = sp.find_transitive_edges(sp.normalize(CI["input_graph"]))
    t0, t1 = {}, {}
    want = sp.simplify(CI["input_graph"], [None], dll=gpu_lib.dll, schedule=[[sp._inv(edge)]], trace=t0)
    assert sp.simplify(CI["input_graph"], [None], dll=gpu_lib.dll, schedule=[[sp._inv(edge)]], trace=t1, topology="device") == want and t1["rounds"] == t0["rounds"]
    with pytest.raises(ValueError):
        sp.simplify(SR["graph"], SR["focal"], dll=gpu_lib.dll, schedule=[[((1, "+"), (3, "+"))]], topology="device")


# ---------------------------------------------------------------- 6. malformed input
def test_malformed_input_fails_the_call_and_leaves_the_library_usable(gpu_lib):
    dll = gpu_lib.dll
    good = tg.graph([(True, "A+ B- C+"), (False, "C+ A+ B-"), (False, "")])
    blocks, paths, nodes = good
    check(dll, good)

    def fails(lists, needle, sched=None):
        with pytest.raises(batch.PgaError, match=needle):
            tp.plan_round(*lists, sched=sched, dll=dll)
        check(dll, good)                                                        # the next call works

    edit = lambda rows, i, **kw: [tuple(kw.get(f, v) for f, v in zip(kw["_f"], r)) if k == i else r for k, r in enumerate(rows)]
    B, P, N = ("id", "len", "depth", "alive"), ("id", "off", "n", "circular"), ("id", "pos0", "pos1", "block", "member", "reverse")
    fails((edit(blocks, 1, _f=B, id=blocks[0][0]), paths, nodes), "strictly ascending")
    fails((blocks, edit(paths, 1, _f=P, id=paths[0][0] - 1), nodes), "path ids")
    fails((blocks, paths, edit(nodes, 2, _f=N, block=3)), "out of range")
    fails((edit(blocks, 2, _f=B, alive=0), paths, nodes), "dead block")
    fails((blocks, paths, edit(nodes, 0, _f=N, member=2)), "member >= depth")
    fails((blocks, edit(paths, 2, _f=P, n=1), nodes), "do not sum")
    fails((blocks, edit(paths, 1, _f=P, off=4), nodes), "running sum")
    fails(good, "not transitive", sched=[(0, 0, 2, 0)])
    fails(good, "not transitive", sched=[(0, 0, 7, 0)])
    fails(good, "twice", sched=[(0, 0, 1, 1), (1, 0, 0, 1)])
    fails(good, "empty schedule", sched=[])
    # found on the device, before any index derived from it is used
    fails((blocks, paths, edit(nodes, 3, _f=N, member=nodes[0][4])) if nodes[3][3] == nodes[0][3] else (blocks, paths, edit(nodes, 4, _f=N, member=nodes[0][4])), "named by")
    twice = (blocks, edit(paths, 2, _f=P, n=1), nodes + [nodes[0]])
    fails(twice, "sum to its depth")                                            # a node that occurs twice on the paths
    fails((edit(blocks, 0, _f=B, depth=3), paths, nodes), "sum to its depth|named by no node")
    # totals of 2^31: the counts are read before any array is
    args = list(tp.pack_lists(*good))
    for at in (0, 2, 4):
        a = list(args)
        a[at] = 1 << 31
        with pytest.raises(batch.PgaError, match="2\\^31"):
            tp.plan_round_raw(a, dll=dll)
    # empty input: empty lists, no device call
    for empty in (([], [], []), (blocks, [], []), (blocks, [(1, 0, 0, 1), (2, 0, 0, 0)], [])):
        got = tp.plan_round(*empty, dll=dll)
        assert got["transitive"] == [] and got["round"] == [] and got["nodes"] is None
    check(dll, good)
