"""pga_join_graphs (pga_join.hip: graph_join on the two flat layouts) against tests/join_gen.py: host_join (the dict union flattened).  Every
comparison is exact in every field of pga_join_out_t, in both flag modes; the output goes on by pointer into pga_reconstruct, pga_plan_simplify,
pga_remove_paths, pga_export_json, a merge round's pga_apply_merge + pga_assemble_blocks and the next pga_join_graphs; two CloseOuts are joined
by pointer; merge_pair runs the real chain.  What each case holds is pinned by tests/test_join_cpu.py."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import apply_gen as ag
import assemble_gen as sg
import close_gen as cg
import join_gen as jg
import reweave_gen as rg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import apply as ap  # noqa: E402
from pangraph_amd import assemble as asm  # noqa: E402
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import close as cl  # noqa: E402
from pangraph_amd import join as jn  # noqa: E402
from pangraph_amd import jsonout  # noqa: E402
from pangraph_amd import remove as rm  # noqa: E402
from pangraph_amd import topology as tp  # noqa: E402
from test_gpu_assemble import _path_sequences  # noqa: E402
from test_gpu_close import as_json  # noqa: E402
from test_join_cpu import conflict_parts, split  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
pad16 = lambda n: (n + 15) // 16 * 16


def check(dll, k, name=""):
    for flags in (0, jn.COPY_CONSENSUS):
        got = jn.join_graphs([p["t"] for p in k["parts"]], flags, dll=dll)
        assert jg.same(got, k["exp"]) is None, (name, flags, jg.same(got, k["exp"]), got["totals"], k["exp"]["totals"])
        assert got["totals"][9] == (sum(pad16(b[1]) for b in k["exp"]["blocks"]) if flags else 0), (name, flags)


# ---------------------------------------------------------------- 1. the named cases and seeded random joins, both modes
@pytest.mark.parametrize("name", sorted(jg.CASES))
def test_named_case(gpu_lib, name):
    check(gpu_lib.dll, jg.case(name), name)


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_joins(gpu_lib, seeds):
    for seed in seeds:
        check(gpu_lib.dll, jg.random_case(seed), seed)


def test_every_part_empty_makes_no_device_call(gpu_lib):
    empty = jg.tables_of(copy.deepcopy(jg.EMPTY))
    got = jn.join_graphs([empty, empty, empty], dll=gpu_lib.dll)
    assert got["totals"] == (0, 0, 0, 0, 3, 0, 0, 0, 0, 0) and got["block_map_off"] == [0, 0, 0, 0] and got["blocks"] == []


def test_consensus_pointers(gpu_lib):
    """with PGA_JOIN_COPY_CONSENSUS every consensus pointer leads into out->cons, at a multiple of 16; without it into the part's own letters"""
    k = jg.case("alternating")
    for flags in (0, jn.COPY_CONSENSUS):
        K = [jn.Tables(p["t"]) for p in k["parts"]]
        out = jn.join_graphs_raw(K, flags=flags, dll=gpu_lib.dll)
        try:
            o = out.out
            base = C.addressof(o.cons.contents)
            inside = [0 <= cl._addr(o.rc_blocks[i]) - base < max(o.n_cons_letters, 1) and (cl._addr(o.rc_blocks[i]) - base) % 16 == 0 for i in range(o.n_blocks)]
            assert inside == [bool(flags)] * o.n_blocks
            if not flags:
                src = {K[p].graph[1][b].block_id: cl._addr(K[p].B[b]) for p in range(2) for b in range(K[p].n_blocks)}
                assert all(cl._addr(o.rc_blocks[i]) == src[o.blocks[i].block_id] for i in range(o.n_blocks) if o.blocks[i].cons_len)
        finally:
            out.free()


# ---------------------------------------------------------------- 2. the output goes on by pointer
def joined_graph(k):
    g = copy.deepcopy(jg.EMPTY)
    for p in k["parts"]:
        g = jn.graph_join(g, p["g"])
    return g


@pytest.mark.parametrize("flags", [0, jn.COPY_CONSENSUS])
def test_output_goes_to_reconstruct_plan_simplify_remove_and_json(gpu_lib, flags):
    dll = gpu_lib.dll
    for name, k in [(x, jg.case(x)) for x in jg.SMALL] + [(s, jg.random_case(s)) for s in range(10)]:
        K = [jn.Tables(p["t"]) for p in k["parts"]]
        out = jn.join_graphs_raw(K, flags=flags, dll=dll)
        try:
            e = k["exp"]
            lists = (e["blocks"], e["paths"], e["nodes"])
            # pga_reconstruct in verify mode against the sequences the paths spell in their own parts
            want_seq = [None] * len(e["paths"])
            for j, (P, p) in enumerate(zip(K, k["parts"])):
                seqs = _path_sequences(dll, P.block_args(), (p["t"]["blocks"], p["t"]["paths"], p["t"]["nodes"]))
                for i, s in enumerate(seqs):
                    want_seq[e["path_map"][e["path_map_off"][j] + i]] = s
            assert all(v == (0, 0) for v in _path_sequences(dll, out.block_args(), lists, want_seq)), name
            want_graph = tp.pack_lists(*lists)
            got_plan, want_plan = tp.plan_round_raw(out.graph_args(), dll=dll), tp.plan_round_raw(want_graph, dll=dll, keep=want_graph)
            try:
                assert got_plan.to_lists() == want_plan.to_lists(), name
            finally:
                got_plan.free(); want_plan.free()
            removed = rm.remove_paths_raw(out.graph_args(), out.block_args(), [1] * len(e["paths"]), rm.COMPACT_LETTERS, out.out.n_ins_letters, dll=dll)
            try:
                r = removed.to_lists()
                assert (r["blocks"], r["paths"], r["nodes"]) == lists and r["members"] == [tuple(c) for c in e["counts"].tolist()] and (r["ins_seq"] or b"") == e["ins_seq"], name
                assert r["inss"] == [tuple(x) for x in e["inss"].tolist()] and r["subs"] == [tuple(x) for x in e["subs"].tolist()], name
            finally:
                removed.free()
            after = joined_graph(k)
            path_meta = [(after["paths"][pid]["tot_len"], (after["paths"][pid]["name"] or "").encode(), None) for pid in sorted(after["paths"])]
            pieces = []
            jsonout.export_json_raw(out.graph_args(), out.block_args(), path_meta, pieces.append, out.out.n_ins_letters, dll=dll).free()
            for p in after["paths"].values():
                p["name"] = p["name"] or ""
            assert b"".join(pieces) == jsonout.json_tables(as_json(after))["text"], name
        finally:
            out.free()


def shifted_tables(t, d_block, d_path, d_node):
    t = dict(t)
    t["blocks"] = [(b[0] + d_block,) + tuple(b[1:]) for b in t["blocks"]]
    t["paths"] = [(p[0] + d_path,) + tuple(p[1:]) for p in t["paths"]]
    t["nodes"] = [(n[0] + d_node,) + tuple(n[1:]) for n in t["nodes"]]
    t["who"] = [(w[0] + d_node, w[1]) for w in t["who"]]
    return t


def test_two_close_outs_joined_by_pointer_feed_a_merge_round(gpu_lib):
    """CloseOut x 2 -> JoinOut -> pga_apply_merge + pga_assemble_blocks, every step by pointer, exact against the dict route"""
    dll = gpu_lib.dll
    ka, kb = cg.case("letters"), cg.case("no_update")
    tb = shifted_tables(kb["t"], 1000, 100, 1_000_000)
    gb = jg.relabel({f: kb["spec"][f] for f in ("blocks", "nodes", "paths")}, block=lambda b: b + 1000, path=lambda p: p + 100, node=lambda n: n + 1_000_000)
    parts = [{"g": ka["after"], "t": ka["exp"]}, {"g": gb, "t": cg.flat_close(tb)}]
    e1 = jg.host_join(parts)
    after = jn.graph_join(ka["after"], gb)
    assert len(e1["ins_seq"]) >= sg.POOL
    KA, KB = cl.Tables(ka["t"]), cl.Tables(tb)
    first_a = cl.close_round_raw(*KA.call_args(), dll=dll, keep=KA)
    first_b = cl.close_round_raw(*KB.call_args(), dll=dll, keep=KB)
    joined = jn.join_graphs_raw([first_a, first_b], dll=dll)
    try:
        assert first_b.n_upd == 0 and jg.same(joined.to_lists(), e1) is None, jg.same(joined.to_lists(), e1)
        cut_id = [b[0] for b in e1["blocks"] if b[2] >= 2 and b[1] >= 20][0]
        c2 = ag.synth_graph(copy.deepcopy(after), {cut_id: ag.pieces(2, 10, 1 << 40)})
        off = np.zeros((len(e1["counts"]) + 1, 3), np.int64)
        off[1:] = np.cumsum(e1["counts"].astype(np.int64), axis=0)
        member = lambda rng, i: tuple(e1[f][off[i, q]:off[i + 1, q]].copy() for q, f in enumerate(("subs", "dels", "inss")))
        k2 = sg.build(c2, 60, before=member, pool0=e1["ins_seq"])
        assert k2["t"]["counts"].tolist() == e1["counts"].tolist() and list(c2["args"][0]) == e1["blocks"] and list(c2["args"][2]) == e1["nodes"]
        K2 = asm.Tables(k2["t"])
        _, plan, sliced, promised, _ = K2.call_args()
        cut = ap.pack_cut_lists(*c2["args"][3:])
        applied = ap.apply_merge_raw(joined.graph_args(), *cut, dll=dll, keep=cut)
        try:
            assert tp.unpack_lists(applied.graph_args()) == tuple([tuple(x) for x in c2["exp"][f]] for f in ("blocks", "paths", "nodes"))
            second = asm.assemble_blocks_raw(joined.block_args(), plan, sliced, promised, applied, dll=dll, keep=K2, ins_seq_len=joined.out.n_ins_letters)
            try:
                assert sg.same(second.to_arrays(), k2["exp"][0]) is None, sg.same(second.to_arrays(), k2["exp"][0])
            finally:
                second.free()
        finally:
            applied.free()
    finally:
        joined.free(); first_b.free(); first_a.free()


def test_a_join_out_is_joined_again(gpu_lib):
    dll = gpu_lib.dll
    k = jg.case("three_parts")
    K = [jn.Tables(p["t"]) for p in k["parts"]]
    first = jn.join_graphs_raw(K[:2], dll=dll)
    try:
        e01 = jg.host_join(k["parts"][:2])
        assert jg.same(first.to_lists(), e01) is None
        want = jg.host_join([{"g": jn.graph_join(k["parts"][0]["g"], k["parts"][1]["g"]), "t": e01}, k["parts"][2]])
        for flags in (0, jn.COPY_CONSENSUS):
            second = jn.join_graphs_raw([first, K[2]], flags=flags, dll=dll)
            try:
                got = second.to_lists()
                assert jg.same(got, want) is None, jg.same(got, want)
                for f in ("blocks", "paths", "nodes", "rc_blocks", "who", "ins_seq"):   # the same graph as the three parts joined at once
                    assert got[f] == k["exp"][f], f
            finally:
                second.free()
    finally:
        first.free()


# ---------------------------------------------------------------- 3. merge_pair with the real chain behind it
def test_merge_pair_on_the_device_against_the_dict_route(gpu_lib, oracle_lib):
    import promise_ref as pr
    from test_gpu_close import _round
    dll = gpu_lib.dll
    solve = lambda promises: [pr.solve_promise(oracle_lib.dll, q) for q in promises]

    def both(make, thr):
        (l0, r0, matches), (l1, r1, _) = make(), make()
        want = _round(lambda: jn.merge_pair(l0, r0, [matches], thr, solve=solve, dll=dll))
        got = _round(lambda: jn.merge_pair(l1, r1, [matches], thr, join="device", close="device", dll=dll))
        assert got == want
        return want

    def from_vector():
        g, matches = rg.reference_graph(VEC)
        return split(g) + (matches,)

    def from_random(seed):
        left, matches = ag.random_graph(seed)
        return left, jg.relabel(jg.graph(seed, {50: (20, 3), 60: (30, 2)}), path=lambda p: 3 * p), matches

    assert both(from_vector, VEC["reweave"]["thr_len"]) not in ("MergeError", "CloseError")
    done = [both(lambda: from_random(seed), rg.THR) not in ("MergeError", "CloseError") for seed in range(12)]
    assert sum(done) >= 2


# ---------------------------------------------------------------- 4. conflicts and malformed input: -1, a message, a zeroed output
def _refused(dll, parts, flags=0):
    with pytest.raises(batch.PgaError) as e:
        jn.join_graphs_raw(parts, flags=flags, dll=dll).free()
    assert str(e.value).startswith("pga_join_graphs: ")
    return str(e.value)[len("pga_join_graphs: "):]


@pytest.mark.parametrize("kind", ["block", "path", "node", "node_within"])
def test_conflicting_keys(gpu_lib, kind):
    tables, ident = conflict_parts(kind)
    where = "parts 1 and 1" if kind == "node_within" else "parts 0 and 1"
    assert _refused(gpu_lib.dll, [jn.Tables(t) for t in tables]) == f"Conflicting key: {kind.split('_')[0]} id {ident} is present twice ({where})"


def test_the_smallest_conflicting_id_is_named(gpu_lib):
    tables = [copy.deepcopy(p["t"]) for p in jg.case("alternating")["parts"]]
    a, b = tables
    b["nodes"][2], b["nodes"][7] = (a["nodes"][3][0],) + tuple(b["nodes"][2][1:]), (a["nodes"][9][0],) + tuple(b["nodes"][7][1:])
    assert f"node id {min(a['nodes'][3][0], a['nodes'][9][0])} " in _refused(gpu_lib.dll, [jn.Tables(t) for t in tables])


def _alive(K, which=0):
    return [b for b in range(K.n_blocks) if K.graph[1][b].alive][which]


def _slot_twice(K):
    """node 1 of part 1 takes the slot of another node of its block: its own slot is then named by no node, the other by two -> the message about the lower
    of the two slots (in the part), which is the one reported"""
    N, B = K[1].graph[5], K[1].graph[1]
    j = [i for i in range(K[1].graph[4]) if i != 1 and N[i].block == N[1].block][0]
    first = sum(B[b].depth for b in range(N[j].block) if B[b].alive)
    left, taken = first + N[1].member, first + N[j].member
    N[1].member = N[j].member
    return f"named by no node (slot {left})" if left < taken else f"named by two nodes (slot {taken})"


HOST = [
    (lambda K: setattr(K[1].graph[1][_alive(K[1], 1)], "block_id", K[1].graph[1][_alive(K[1], 0)].block_id), lambda K: f"part 1: the ids of the alive blocks are not strictly ascending (block {_alive(K[1], 1)})"),
    (lambda K: setattr(K[1].graph[3][1], "path_id", K[1].graph[3][0].path_id), lambda K: "part 1: the path ids are not ascending (path 1)"),
    (lambda K: setattr(K[0].graph[1][K[0].graph[5][0].block], "alive", 0), lambda K: "part 0: a node names a dead block (node 0)"),
    (lambda K: setattr(K[1].graph[5][0], "block", K[1].n_blocks), lambda K: "part 1: a node names a block out of range (node 0)"),
    (lambda K: setattr(K[0].graph[5][0], "member", 99), lambda K: "part 0: member >= depth (node 0)"),
    (lambda K: setattr(K[1].graph[3][1], "node_off", K[1].graph[3][1].node_off + 1), lambda K: "part 1: node_off is not the running sum of n_nodes (path 1)"),
    (lambda K: setattr(K[1].B[_alive(K[1])], "n_members", K[1].B[_alive(K[1])].n_members + 1), lambda K: f"part 1: n_members of a block differs from its depth (block {_alive(K[1])})"),
    (lambda K: setattr(K[0].B[_alive(K[0])], "cons_len", K[0].B[_alive(K[0])].cons_len + 1), lambda K: f"part 0: cons_len of a block differs between the graph and the block arrays (block {_alive(K[0])})"),
    (lambda K: setattr(K[1], "M", np.zeros((0, 3), np.uint32)), lambda K: "part 1: null argument or negative count"),
    (lambda K: setattr(K[0], "W", np.zeros(0, asm.WHO)), lambda K: "part 0: null argument or negative count"),
]


@pytest.mark.parametrize("at", range(len(HOST)))
def test_refused_on_the_host(gpu_lib, at):
    change, message = HOST[at]
    K = [jn.Tables(copy.deepcopy(p["t"])) for p in jg.case("alternating")["parts"]]
    change(K)
    assert _refused(gpu_lib.dll, K) == message(K)


def test_unknown_flag_and_no_part(gpu_lib):
    K = [jn.Tables(p["t"]) for p in jg.case("two_singletons")["parts"]]
    assert _refused(gpu_lib.dll, K, flags=2) == "unknown flag"
    assert _refused(gpu_lib.dll, []) == "n_parts < 1"


def test_a_slot_named_twice(gpu_lib):
    K = [jn.Tables(copy.deepcopy(p["t"])) for p in jg.case("alternating")["parts"]]
    what = _slot_twice(K)
    assert _refused(gpu_lib.dll, K) == f"part 1: a (block, member) slot is {what}"


def test_an_insertion_beyond_its_own_part_but_inside_the_concatenated_letters(gpu_lib):
    k = jg.case("buffer_end")
    K = [jn.Tables(copy.deepcopy(p["t"])) for p in k["parts"]]
    assert len(K[0].L) + len(K[1].L) > len(K[0].L) + 1                             # (the letters of part 1 lie behind part 0's on the device)
    K[0].I["seq_off"][-1] += 1
    assert _refused(gpu_lib.dll, K) == f"part 0: seq_off + len of an insertion lies beyond its part's letter buffer (insertion {len(K[0].I) - 1})"
    K = [jn.Tables(copy.deepcopy(p["t"])) for p in k["parts"]]
    assert _refused(gpu_lib.dll, [K[0], (K[1], K[1].W, 2)]) == "part 1: seq_off + len of an insertion lies beyond its part's letter buffer (insertion 0)"
    K = [jn.Tables(copy.deepcopy(p["t"])) for p in k["parts"]]
    K[1].I["seq_off"][0] = (1 << 64) - 2                                          # (seq_off + len wraps)
    assert _refused(gpu_lib.dll, K) == "part 1: seq_off + len of an insertion lies beyond its part's letter buffer (insertion 0)"


def test_a_refusal_zeroes_the_output(gpu_lib):
    dll = gpu_lib.dll
    jn._bind(dll)
    tables, _ = conflict_parts("block")
    K = [jn.Tables(t) for t in tables]
    P = jn.pack_parts(K)
    out = jn.join_out_t()
    C.memset(C.byref(out), 0x5a, C.sizeof(out))
    assert dll.pga_join_graphs(2, asm._ptr(P), 0, C.byref(out)) == -1 and bytes(out) == bytes(C.sizeof(out))


def test_last_ms_reports_the_three_phases(gpu_lib):
    jn.join_graphs([p["t"] for p in jg.case("straddle")["parts"]], dll=gpu_lib.dll)
    ms = jn.last_ms(gpu_lib.dll)
    assert len(ms) == 3 and all(x >= 0 for x in ms) and sum(ms) > 0
