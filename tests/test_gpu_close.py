"""pga_close_round (pga_close.hip: the tail of a self-merge round folded back into the flat graph and the block arrays) against
tests/close_gen.py: host_close (the dict graph after detach_unaligned_nodes, the block replacement and the second detach_unaligned_nodes,
flattened).  Every comparison is exact in every field of pga_close_out_t, in both flag modes; the output goes on by pointer into
pga_reconstruct, pga_plan_simplify, pga_remove_paths, pga_export_json and a second round's pga_apply_merge + pga_assemble_blocks; the real
chain runs on the reference's reweave vector and on random graphs.  What each case holds is pinned by tests/test_close_cpu.py."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import apply_gen as ag
import assemble_gen as sg
import close_gen as cg
import reweave_gen as rg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import apply as ap  # noqa: E402
from pangraph_amd import assemble as asm  # noqa: E402
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import close as cl  # noqa: E402
from pangraph_amd import jsonout  # noqa: E402
from pangraph_amd import remove as rm  # noqa: E402
from pangraph_amd import topology as tp  # noqa: E402
from pangraph_amd.reconstruct import _Packed  # noqa: E402
from test_gpu_assemble import _path_sequences  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))
pad16 = lambda n: (n + 15) // 16 * 16


def owned_letters(k, flags):
    """the bytes of out->cons: every alive block with the flag, otherwise the updated blocks of kind 1 and 2 and the singletons"""
    e, t = k["exp"], k["t"]
    if flags:
        return sum(pad16(b[1]) for b in e["blocks"])
    made = {e["block_map"][b] for j, b in enumerate(t["upd"]) if t["rc"]["blocks"][j][0]} | {o[3] for o in e["orphans"]}
    return sum(pad16(e["blocks"][i][1]) for i in made)


def check(dll, k, name=""):
    for flags in (0, cl.COPY_CONSENSUS):
        got = cl.close_round(k["t"], flags, dll=dll)
        assert cg.same(got, k["exp"]) is None, (name, flags, cg.same(got, k["exp"]), got["totals"], k["exp"]["totals"])
        assert got["totals"][9] == owned_letters(k, flags), (name, flags)


# ---------------------------------------------------------------- 1. the named cases and seeded random rounds, both modes
@pytest.mark.parametrize("name", sorted(cg.CASES))
def test_named_case(gpu_lib, name):
    check(gpu_lib.dll, cg.case(name), name)


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_rounds(gpu_lib, seeds):
    for seed in seeds:
        check(gpu_lib.dll, cg.random_case(seed), seed)


def test_copied_consensus_needs_only_the_output(gpu_lib):
    """with PGA_CLOSE_COPY_CONSENSUS every consensus pointer leads into out->cons, at a multiple of 16; without it the survivors' lead into the caller's letters"""
    k = cg.case("both_in_one_block")
    for flags in (0, cl.COPY_CONSENSUS):
        K = cl.Tables(k["t"])
        out = cl.close_round_raw(*K.call_args(), flags=flags, dll=gpu_lib.dll, keep=K)
        try:
            o = out.out
            base = C.addressof(o.cons.contents)
            inside = [0 <= cl._addr(o.rc_blocks[i]) - base < max(o.n_cons_letters, 1) and (cl._addr(o.rc_blocks[i]) - base) % 16 == 0 for i in range(o.n_blocks)]
            made = {k["exp"]["block_map"][b] for b in k["t"]["upd"]} | {r[3] for r in k["exp"]["orphans"]}
            assert inside == ([True] * o.n_blocks if flags else [i in made for i in range(o.n_blocks)])
        finally:
            out.free()


# ---------------------------------------------------------------- 2. the output goes on by pointer
def as_json(g):
    edit = lambda e: {"subs": [{"pos": p, "alt": a} for p, a in e["subs"]], "dels": [{"pos": p, "len": n} for p, n in e["dels"]], "inss": [{"pos": p, "seq": s} for p, s in e["inss"]]}
    return {"paths": {str(k): dict(p, desc=None) for k, p in g["paths"].items()}, "nodes": {str(k): dict(n, position=list(n["position"])) for k, n in g["nodes"].items()},
            "blocks": {str(k): {"consensus": b["consensus"], "alignments": {str(n): edit(e) for n, e in b["alignments"].items()}} for k, b in g["blocks"].items()}}


def packed_after(k):
    """the blocks after packed from host_close's dict graph, in id order, members in node-id order"""
    after = k["after"]
    return _Packed([{"consensus": after["blocks"][b]["consensus"], "members": [after["blocks"][b]["alignments"][n] for n in sorted(after["blocks"][b]["alignments"])]} for b in sorted(after["blocks"])], [])


@pytest.mark.parametrize("flags", [0, cl.COPY_CONSENSUS])
def test_output_goes_to_reconstruct_plan_simplify_remove_and_json(gpu_lib, flags):
    dll = gpu_lib.dll
    n = 0
    for name, k in [(x, cg.case(x)) for x in cg.SMALL] + [(s, cg.random_case(s)) for s in range(10)]:
        K = cl.Tables(k["t"])
        out = cl.close_round_raw(*K.call_args(), flags=flags, dll=dll, keep=K)
        try:
            e = k["exp"]
            lists = (e["blocks"], e["paths"], e["nodes"])
            K2 = packed_after(k)
            assert _path_sequences(dll, out.block_args(), lists) == _path_sequences(dll, K2.args()[:7], lists), name
            want_graph = tp.pack_lists(*lists)
            got_plan, want_plan = tp.plan_round_raw(out.graph_args(), dll=dll), tp.plan_round_raw(want_graph, dll=dll, keep=want_graph)
            try:
                assert got_plan.to_lists() == want_plan.to_lists(), name
            finally:
                got_plan.free(); want_plan.free()
            removed = rm.remove_paths_raw(out.graph_args(), out.block_args(), [1] * len(e["paths"]), rm.COMPACT_LETTERS, out.out.n_ins_letters, dll=dll)
            try:
                r = removed.to_lists()
                assert (r["blocks"], r["paths"], r["nodes"]) == lists and r["members"] == [tuple(c) for c in e["counts"].tolist()] and r["ins_seq"] == e["ins_seq"], name
                assert r["inss"] == [tuple(x) for x in e["inss"].tolist()] and r["subs"] == [tuple(x) for x in e["subs"].tolist()], name
            finally:
                removed.free()
            after = k["after"]

            class View:
                graph_args, block_args = out.graph_args(), out.block_args()
                path_meta = [(after["paths"][pid]["tot_len"], after["paths"][pid]["name"].encode(), None) for pid in sorted(after["paths"])]
                ins_seq_len = out.out.n_ins_letters
            pieces = []
            j = jsonout.export_json_raw(View.graph_args, View.block_args, View.path_meta, pieces.append, View.ins_seq_len, dll=dll)
            j.free()
            assert b"".join(pieces) == jsonout.json_tables(as_json(after))["text"], name
            n += out.out.n_orphans
        finally:
            out.free()
    assert n >= 30


def test_output_is_the_graph_before_of_a_second_round(gpu_lib):
    """round 2's pga_apply_merge and pga_assemble_blocks take the CloseOut's two layouts by pointer"""
    dll = gpu_lib.dll
    k = cg.case("letters")
    e1, after = k["exp"], k["after"]
    assert len(e1["ins_seq"]) >= sg.POOL
    cut_id = [b[0] for b in e1["blocks"] if b[2] >= 2 and b[1] >= 20][0]
    c2 = ag.synth_graph(copy.deepcopy(after), {cut_id: ag.pieces(2, 10, 1 << 40)})
    off = np.zeros((len(e1["counts"]) + 1, 3), np.int64)
    off[1:] = np.cumsum(e1["counts"].astype(np.int64), axis=0)
    member = lambda rng, i: tuple(e1[f][off[i, q]:off[i + 1, q]].copy() for q, f in enumerate(("subs", "dels", "inss")))
    k2 = sg.build(c2, 60, before=member, pool0=e1["ins_seq"])
    assert k2["t"]["counts"].tolist() == e1["counts"].tolist() and list(c2["args"][0]) == e1["blocks"] and list(c2["args"][2]) == e1["nodes"]
    K1, K2 = cl.Tables(k["t"]), asm.Tables(k2["t"])
    first = cl.close_round_raw(*K1.call_args(), dll=dll, keep=K1)
    try:
        _, plan, sliced, promised, _ = K2.call_args()
        cut = ap.pack_cut_lists(*c2["args"][3:])                                  # (assemble.Tables keeps no member slots: the cut of the apply call is packed from the case)
        applied = ap.apply_merge_raw(first.graph_args(), *cut, dll=dll, keep=cut)
        try:
            got = tp.unpack_lists(applied.graph_args())
            assert got == tuple([tuple(x) for x in c2["exp"][f]] for f in ("blocks", "paths", "nodes"))
            second = asm.assemble_blocks_raw(first.block_args(), plan, sliced, promised, applied, dll=dll, keep=K2, ins_seq_len=first.out.n_ins_letters)
            try:
                assert sg.same(second.to_arrays(), k2["exp"][0]) is None, sg.same(second.to_arrays(), k2["exp"][0])
            finally:
                second.free()
        finally:
            applied.free()
    finally:
        first.free()


# ---------------------------------------------------------------- 3. the real chain against the tail in dicts
def _canon(g):
    edit = lambda e: {f: [tuple(x) for x in e[f]] for f in ("subs", "dels", "inss")}
    return {"paths": {p: dict(v, nodes=list(v["nodes"])) for p, v in g["paths"].items()}, "nodes": {n: dict(v, position=tuple(v["position"])) for n, v in g["nodes"].items()},
            "blocks": {b: {"consensus": v["consensus"], "alignments": {n: edit(e) for n, e in v["alignments"].items()}} for b, v in g["blocks"].items()}}


def _round(run):
    try:
        return _canon(run())
    except asm.MergeError:
        return "MergeError"
    except cl.CloseError:
        return "CloseError"


def test_self_merge_round_on_the_device_against_the_tail_in_dicts(gpu_lib, oracle_lib):
    import promise_ref as pr
    dll = gpu_lib.dll
    solve = lambda promises: [pr.solve_promise(oracle_lib.dll, q) for q in promises]
    verified = []

    def verify(closed, applied, assembled):
        """pga_reconstruct takes the CloseOut by pointer, in verify mode against the sequences the paths spelled before the tail"""
        before = _path_sequences(dll, assembled.block_args(), tp.unpack_lists(applied.graph_args()))
        verified.append(_path_sequences(dll, closed.block_args(), tp.unpack_lists(closed.graph_args()), before))

    thr = VEC["reweave"]["thr_len"]
    g0, matches = rg.reference_graph(VEC)
    g1, _ = rg.reference_graph(VEC)
    want = _round(lambda: cl.self_merge_round(g0, matches, thr, solve=solve, dll=dll))
    got = _round(lambda: cl.self_merge_round(g1, matches, thr, close="device", dll=dll, tap=verify))
    assert got == want and want not in ("MergeError", "CloseError")
    n_done, orphans = 0, []
    for seed in range(40):                                                       # (random letters under random CIGARs: most rounds end in solve_promise's Err, on both sides)
        g, ms = ag.random_graph(seed)
        want = _round(lambda: cl.self_merge_round(ag.random_graph(seed)[0], ms, rg.THR, solve=solve, dll=dll))
        got = _round(lambda: cl.self_merge_round(g, ms, rg.THR, close="device", dll=dll, tap=lambda c, a, b: (orphans.append(c.out.n_orphans), verify(c, a, b))))
        assert got == want, seed
        n_done += want not in ("MergeError", "CloseError")
    print(f"real chain: {n_done} of 40 random rounds completed, {len(orphans)} reached pga_close_round, orphans per round {orphans}")
    assert n_done >= 6 and len(verified) >= 1 + n_done and all(v == (0, 0) for per in verified for v in per)


def test_device_tail_on_generated_rounds_against_the_tail_in_dicts(gpu_lib):
    """the real pga_detach_unaligned -> pga_reconsensus -> pga_detach_unaligned -> pga_close_round by pointer on the generated graphs, whose
    members leave by their own edits, against detach_graph / reconsensus / detach_graph on dicts: here orphans do go through the real chain
    (the random merge rounds above end without one)"""
    from pangraph_amd import detach as dt
    dll = gpu_lib.dll
    n_done, orphans, kinds = 0, 0, set()

    def count(res):
        nonlocal orphans
        orphans += res.out.n_orphans
        kinds.update(res.out.kinds[:res.n_upd])

    def run(f):
        try:
            return _canon(f())
        except (cl.CloseError, dt.DetachError):
            return "Err"

    for name, k in [(x, cg.case(x)) for x in cg.SMALL if cg.case(x)["spec"]["upd"]] + [(s, cg.random_case(s)) for s in range(40) if cg.random_case(s)["spec"]["upd"]]:
        spec = k["spec"]
        graph = lambda: copy.deepcopy({f: spec[f] for f in ("blocks", "nodes", "paths")})
        want = run(lambda: cl._host_tail(graph(), list(spec["upd"]), dll))
        K = cl.Tables({f: v for f, v in k["t"].items() if f not in ("detached", "rc", "redetached")} | {"upd": []})
        o = asm.assemble_out_t()
        o.n_blocks, o.n_members, o.n_subs, o.n_dels, o.n_inss, o.n_ins_letters = K.n_blocks, len(K.W), len(K.S), len(K.D), len(K.I), len(K.L)
        o.blocks = C.cast(K.B, type(o.blocks)); o.ins_seq = C.cast(C.c_char_p(K.L), type(o.ins_seq))
        for field, arr in (("members", K.M), ("subs", K.S), ("dels", K.D), ("inss", K.I), ("who", K.W)):
            if arr.size:
                setattr(o, field, C.cast(C.c_void_p(arr.ctypes.data), type(getattr(o, field))))
        got = run(lambda: cl.device_tail(graph(), K.graph, o, k["t"]["upd"], dll, tap=count))
        assert got == want, name
        n_done += want != "Err"
    print(f"device tail on generated rounds: {n_done} completed, {orphans} orphans, kinds {sorted(kinds)}")
    assert n_done >= 10 and orphans >= 10


# ---------------------------------------------------------------- 4. malformed input: -1, a message, a zeroed output
def _raw(dll, name, change, flags=0):
    """the call on the tables of a case after change(K) -> the message of the refusal"""
    K = cl.Tables(copy.deepcopy(cg.case(name)["t"]))
    args = list(K.call_args())
    res = change(K, args)
    if res is not None:
        args = res
    with pytest.raises(batch.PgaError) as e:
        cl.close_round_raw(*args, flags=flags, dll=dll, keep=K).free()
    assert str(e.value).startswith("pga_close_round: ")
    return str(e.value)


def _set(args, i, v):
    args[i] = v
    return args


HOST = [
    ("both_in_one_block", lambda K, a: _set(a, 4, [K.n_blocks]), "an updated block is out of range (updated block 0)"),
    ("first_only", lambda K, a: _set(a, 4, [a[4][0], a[4][0]]), "an updated block is named twice (updated block 1)"),
    ("dead_entries", lambda K, a: _set(a, 4, [0]), "an updated block is dead (updated block 0)"),
    ("both_in_one_block", lambda K, a: setattr(K.B[0], "n_members", K.B[0].n_members + 1), "n_members of a block differs from its depth (block 0)"),
    ("both_in_one_block", lambda K, a: setattr(K.d1.out, "n_blocks", K.d1.out.n_blocks + 1), "detached->n_blocks is not n_upd + its orphans"),
    ("both_in_one_block", lambda K, a: setattr(K.d2.out, "n_blocks", K.d2.out.n_blocks - 1), "redetached->n_blocks is not n_upd + its orphans"),
    ("both_in_one_block", lambda K, a: setattr(K.RB[0], "kind", -3), "the reconsensus failed for a block (updated block 0, kind -3)"),
    ("both_in_one_block", lambda K, a: setattr(K.RM[1], "status", 7), "status other than 0 (updated block 0, member 1, status 7)"),
    ("both_in_one_block", lambda K, a: K.d1.O.__setitem__(0, tuple(K.d1.O[0])[:5] + (2, 0)), "an orphan's sequence was not built: its record has a status other than 0 (first detach, orphan 0, status 2)"),
    ("both_in_one_block", lambda K, a: K.d2.O.__setitem__(1, tuple(K.d2.O[1])[:5] + (3, 0)), "(second detach, orphan 1, status 3)"),
    ("both_in_one_block", lambda K, a: setattr(K.B[0], "cons_len", K.B[0].cons_len + 1), "cons_len of a block differs between the graph and the block arrays (block 0)"),
    ("no_orphan", lambda K, a: setattr(K.RB[[j for j in range(3) if K.RB[j].kind == 0][0]], "cons_len", 7), "a kind-0 block whose cons_len changed (updated block "),
    ("both_in_one_block", lambda K, a: K.d1.O.__setitem__(0, tuple(K.d1.O[0])[:3] + (0,) + tuple(K.d1.O[0])[4:]), "an orphan record does not name its singleton block (first detach, orphan 0)"),
    ("both_in_one_block", lambda K, a: setattr(K.d2.B[2], "cons_len", K.d2.B[2].cons_len + 1), "an orphan record does not name its singleton block (second detach, orphan 1)"),
    ("both_in_one_block", lambda K, a: setattr(K.graph[5][0], "member", 99), "member >= depth (node 0)"),
    ("both_in_one_block", lambda K, a: setattr(K.graph[3][1], "node_off", 0), "node_off is not the running sum of n_nodes (path 1)"),
    ("both_in_one_block", lambda K, a: _set(a, 3, None), "null argument or negative count"),
    ("both_in_one_block", lambda K, a: _set(a, 5, None), "null argument or negative count"),
    ("first_only", lambda K, a: setattr(K.d1.B[0], "n_members", K.d1.B[0].n_members + 1), "the kept members and the orphans of the first detach are not the members of the updated blocks"),
]


@pytest.mark.parametrize("at", range(len(HOST)))
def test_refused_on_the_host(gpu_lib, at):
    name, change, message = HOST[at]
    assert message in _raw(gpu_lib.dll, name, change)


def test_unknown_flag(gpu_lib):
    assert "unknown flag" in _raw(gpu_lib.dll, "no_orphan", lambda K, a: None, flags=2)


def _swap_kept(K, a):
    m = K.d1.map
    kept = [i for i in range(len(m)) if m[i] < sum(K.d1.B[j].n_members for j in range(len(K.upd)))]
    m[kept[0]], m[kept[1]] = m[kept[1]], m[kept[0]]


def _shift_counts(K, a):
    K.d1.B[0].n_members += 1; K.d1.B[1].n_members -= 1


def _slot_twice_message():
    """node 1 takes node 0's slot: a node of another block leaves its own block short (the counts are reported first), a node of the same block leaves a slot named twice"""
    nodes = cg.case("both_in_one_block")["t"]["nodes"]
    if nodes[0][3] != nodes[1][3]:
        return "the nodes of a block do not sum to its depth (block " + str(min(nodes[0][3], nodes[1][3])) + ")"
    first = sum(b[2] for b in cg.case("both_in_one_block")["t"]["blocks"][:nodes[0][3]])
    return "a (block, member) slot is named by " + ("no node" if nodes[1][4] < nodes[0][4] else "two nodes") + " (slot " + str(first + min(nodes[0][4], nodes[1][4])) + ")"


SLOT_TWICE = _slot_twice_message()
DEVICE = [
    ("first_only", _shift_counts, "do not sum to its depth (first detach, updated block 0)"),
    ("first_only", _swap_kept, "member_map is no bijection onto the kept places and the orphans (first detach, member 0)"),
    # (a kept member whose place leaves the kept range also changes its block's kept count, and the counts are reported first)
    ("first_only", lambda K, a: K.d1.map.__setitem__(0, -1), "do not sum to its depth (first detach, updated block 0)"),
    ("first_only", lambda K, a: K.d1.map.__setitem__(0, len(K.d1.map)), "do not sum to its depth (first detach, updated block 0)"),
    ("first_only", lambda K, a: K.d1.map.__setitem__(1, len(K.d1.map)), "member_map is no bijection onto the kept places and the orphans (first detach, member 1)"),
    ("second_only", lambda K, a: K.d2.map.__setitem__(2, K.d2.map[1]), "member_map is no bijection onto the kept places and the orphans (second detach, member 2)"),
    ("second_only", lambda K, a: setattr(K.RB[0], "kind", 1), "the second detach took a member out of a block that was not realigned (orphan 0 of the second detach)"),
    ("first_only", lambda K, a: K.d1.O.__setitem__(0, tuple(K.d1.O[0])[:2] + (50,) + tuple(K.d1.O[0])[3:]), "Conflicting key: a singleton block_id equals a surviving block's or another singleton's (orphan 0)"),
    ("both_in_one_block", lambda K, a: K.d2.O.__setitem__(0, tuple(K.d2.O[0])[:2] + (int(K.d1.O[1]["block_id"]),) + tuple(K.d2.O[0])[3:]), "Conflicting key"),
    ("both_in_one_block", lambda K, a: (setattr(K.graph[5][1], "block", K.graph[5][0].block), setattr(K.graph[5][1], "member", K.graph[5][0].member)) and None, SLOT_TWICE),
    ("letters", lambda K, a: _set(a, 7, 3), "seq_off + len of an insertion lies beyond its letter buffer (insertion "),
    ("letters", lambda K, a: _set(a, 2, 3), "seq_off + len of an insertion lies beyond its letter buffer (insertion "),
]


@pytest.mark.parametrize("at", range(len(DEVICE)))
def test_refused_on_the_device(gpu_lib, at):
    name, change, message = DEVICE[at]
    got = _raw(gpu_lib.dll, name, change)
    assert message in got, got


def test_a_refusal_zeroes_the_output(gpu_lib):
    dll = gpu_lib.dll
    cl._bind(dll)
    K = cl.Tables(copy.deepcopy(cg.case("first_only")["t"]))
    _shift_counts(K, None)
    graph, block_args, n_letters, who, upd, d1, rc, rc_len, d2 = K.call_args()
    U = np.asarray(upd, np.uint32)
    out = cl.close_out_t()
    C.memset(C.byref(out), 0x5a, C.sizeof(out))
    ptr = asm._ptr
    assert dll.pga_close_round(graph[0], ptr(graph[1]), graph[2], ptr(graph[3]), graph[4], ptr(graph[5]), *[ptr(x) for x in block_args[1:7]], n_letters, ptr(who), len(U), ptr(U),
                               ptr(d1), ptr(rc), rc_len, ptr(d2), 0, C.byref(out)) == -1
    assert bytes(out) == bytes(C.sizeof(out))


def test_last_ms_reports_the_three_phases(gpu_lib):
    cl.close_round(cg.case("straddle")["t"], 0, dll=gpu_lib.dll)
    ms = cl.last_ms(gpu_lib.dll)
    assert len(ms) == 3 and all(x >= 0 for x in ms) and sum(ms) > 0


def test_rc_detach_args_fill_the_second_call(gpu_lib):
    k = cg.case("both_in_one_block")
    K = cl.Tables(k["t"])
    n_kept = sum(k["t"]["detached"]["n_members"])
    for m in range(n_kept):
        K.RM[m].n_subs, K.RM[m].n_dels, K.RM[m].n_inss = m + 1, 2, 3
    merged = [w for j, b in enumerate(k["t"]["upd"]) for w in k["t"]["who"][sum(x[2] for x in k["t"]["blocks"][:b]):sum(x[2] for x in k["t"]["blocks"][:b + 1])]]
    W = (cl.detach_member_t * len(merged))(*[cl.detach_member_t(n, r, 0) for n, r in merged])
    B, M, W2 = cl.rc_detach_args(len(K.upd), K.d1.out, W, K.rc, dll=gpu_lib.dll)
    assert [(B[j].cons_len, B[j].n_members) for j in range(len(K.upd))] == [(len(c), n) for (_, c), n in zip(k["t"]["rc"]["blocks"], k["t"]["detached"]["n_members"])]
    assert cl._addr(B[0]) == C.addressof(K.rc.cons.contents) + K.RB[0].cons_off
    assert [(M[m].n_subs, M[m].n_dels, M[m].n_inss) for m in range(n_kept)] == [(m + 1, 2, 3) for m in range(n_kept)]
    want = {v: merged[m] for m, v in enumerate(k["t"]["detached"]["member_map"]) if v < n_kept}
    assert [(W2[v].node_id, W2[v].reverse) for v in range(n_kept)] == [want[v] for v in range(n_kept)]
