"""pga_assemble_blocks (pga_assemble.hip: the block arrays behind a merge round on the device) against tests/assemble_gen.py: host_assemble (the
dict graph after of the host reweave(), flattened) and, for the merged blocks, detach.merged_blocks (the numpy gather).  Every comparison
is exact in every field: blocks, members, the three lists, letters, who, origin and the totals, in both modes."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

import apply_gen as ag
import assemble_gen as sg
import reweave_gen as rg
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import assemble as asm  # noqa: E402
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import detach as dt  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "reweave_vectors.json")))


def check(dll, k, name=""):
    for flags in (0, asm.MERGED_ONLY):
        got = asm.assemble_blocks(k["t"], flags, dll=dll)
        assert sg.same(got, k["exp"][flags]) is None, (name, flags, sg.same(got, k["exp"][flags]), got["totals"], k["exp"][flags]["totals"])


# ---------------------------------------------------------------- 1. the named cases and seeded random graphs, both modes
@pytest.mark.parametrize("name", sorted(sg.CASES))
def test_named_case(gpu_lib, name):
    check(gpu_lib.dll, sg.case(name), name)


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_graphs(gpu_lib, seeds):
    for seed in seeds:
        check(gpu_lib.dll, sg.random_case(seed), seed)


# ---------------------------------------------------------------- 2. the merged blocks against the numpy gather
def test_merged_only_against_merged_blocks(gpu_lib):
    n = 0
    for name, k in [(x, sg.case(x)) for x in sg.SMALL] + [(s, sg.random_case(s)) for s in range(12)]:
        if not k["t"]["promises"]:
            continue
        assert [q["new_block_id"] for q in k["c"]["promises"]] == sorted(q["new_block_id"] for q in k["c"]["promises"])   # (promise order is new_blocks[] order)
        want = dt.merged_blocks(*sg.merged_blocks_input(k))
        got = asm.assemble_blocks(k["t"], asm.MERGED_ONLY, dll=gpu_lib.dll)
        assert [b[0] for b in got["blocks"]] == [bytes(c) for c in want["cons"]] and [b[1] for b in got["blocks"]] == want["n_members"], name
        assert [w[0] for w in got["who"]] == want["node_ids"].tolist(), name
        assert got["counts"].tolist() == want["counts"].tolist() and got["subs"].tobytes() == want["subs"].tobytes() and got["dels"].tobytes() == want["dels"].tobytes(), name
        assert sg.resolved(got) == sg.resolved(want), name                         # (the two lay the letters out differently)
        n += len(want["cons"])
    assert n >= 20


# ---------------------------------------------------------------- 3. malformed input: refused by message, before the bad index is used
def _corrupt(k, change):
    t = dict(k["t"])
    for f in ("cut", "intervals", "promises", "slices"):
        t[f] = copy.deepcopy(t[f])
    for f in ("s_members", "res", "inss", "p_inss"):
        t[f] = np.array(t[f]).copy()
    t["applied"] = {f: list(v) for f, v in t["applied"].items()}
    change(t)
    return t


def _set(t, table, i, j, v):
    row = list(t[table][i]); row[j] = v; t[table][i] = tuple(row)


def _merged(t):
    return [e for e in t["applied"]["new_blocks"] if e[1] == 1][0]


HOST_REFUSALS = [
    ("a cut block is out of range", lambda t: _set(t, "cut", 0, 0, len(t["blocks"]))),
    ("a cut block is named twice", lambda t: _set(t, "cut", 1, 0, t["cut"][0][0])),
    ("a cut block without intervals", lambda t: _set(t, "cut", 0, 1, 0)),
    ("first_interval is not the running sum", lambda t: _set(t, "cut", 1, 2, t["cut"][1][2] + 1)),
    ("not ascending and disjoint", lambda t: t["intervals"][1].update(start=t["intervals"][0]["end"] - 1)),
    ("beyond its block's consensus", lambda t: t["intervals"][t["cut"][0][1] - 1].update(end=1000)),
    ("do not match members", lambda t: _set(t, "slices", 1, 0, t["slices"][1][0] + 1)),
    ("block_map keeps a cut block", lambda t: t["applied"]["block_map"].__setitem__(t["cut"][0][0], 0)),
    ("neither cut nor mapped", lambda t: t["applied"]["block_map"].__setitem__([i for i, m in enumerate(t["applied"]["block_map"]) if m != ag.NONE][0], ag.NONE)),
    ("a block after is named twice", lambda t: _set(t["applied"], "new_blocks", 1, 0, t["applied"]["new_blocks"][0][0])),
    ("out of range", lambda t: t["applied"]["blocks"].pop()),
    ("not the survivors plus the new blocks", lambda t: t["applied"]["blocks"].append((1 << 63, 1, 0, 1))),
    ("member_off of new_blocks[] is not the running sum", lambda t: _set(t["applied"], "new_blocks", 1, 4, t["applied"]["new_blocks"][1][4] + 1)),
    ("is not the kept members of its slices", lambda t: _set(t["applied"], "blocks", _merged(t)[0], 2, t["applied"]["blocks"][_merged(t)[0]][2] + 1)),
    ("unknown kind", lambda t: _set(t["applied"], "new_blocks", 0, 1, 2)),
    ("is no promise's append_interval", lambda t: t["promises"].pop()),
    ("not an anchor and its append", lambda t: t["promises"].__setitem__(0, (t["promises"][0][1], t["promises"][0][0]))),
    ("n_members of a survivor differs from its depth after", lambda t: _set(t["applied"], "blocks", [m for m in t["applied"]["block_map"] if m != ag.NONE][0], 2, 7)),
    ("applied->n_new_nodes differs", lambda t: t["applied"]["member_src"].append(0)),
]


@pytest.mark.parametrize("at", range(len(HOST_REFUSALS)))
def test_refused_on_the_host(gpu_lib, at):
    message, change = HOST_REFUSALS[at]
    with pytest.raises(batch.PgaError, match="pga_assemble_blocks: .*" + message.replace("[", r"\[").replace("]", r"\]")):
        asm.assemble_blocks(_corrupt(sg.case("alternating"), change), dll=gpu_lib.dll)


def test_unknown_flag(gpu_lib):
    with pytest.raises(batch.PgaError, match="unknown flag"):
        asm.assemble_blocks(sg.case("alternating")["t"], 2, dll=gpu_lib.dll)


def _first_append_row(t):
    """(the place in member_src, the member of its promise) of the first append member of the merged block"""
    e = _merged(t)
    q = t["slices"][e[3]]
    for s in range(e[4], e[4] + 8):
        if q[0] <= t["applied"]["member_src"][s] < q[0] + q[1]:
            return s, t["applied"]["member_src"][s] - q[0]


def _status(t):
    t["res"][_first_append_row(t)[1]][0] = 3


DEVICE_REFUSALS = [
    ("a member_src entry lies outside the slices of its block", lambda t: t["applied"]["member_src"].__setitem__(_merged(t)[4], t["applied"]["member_src"][[e for e in t["applied"]["new_blocks"] if e[1] == 0][0][4]])),   # (another block's member)
    ("a member_src entry lies outside the slices of its block", lambda t: t["applied"]["member_src"].__setitem__(_merged(t)[4], (1 << 64) - 1)),
    ("a member_src entry is used twice", lambda t: t["applied"]["member_src"].__setitem__(_merged(t)[4], t["applied"]["member_src"][_merged(t)[4] + 1])),
    (r"status other than 0 \(promise 0, member \d+; member \d+ after\)", _status),
    ("a source offset \\+ count lies beyond its list", lambda t: t["res"][0].__setitem__(4, (1 << 63) - 10)),
    ("a source offset \\+ count lies beyond its list", lambda t: t["s_members"][0].__setitem__(5, len(t["s_inss"]) + 1)),
    ("lies beyond its letter buffer", lambda t: t.update(ins_seq=t["ins_seq"][:3])),
    ("lies beyond its letter buffer", lambda t: t.update(p_ins_seq=b"")),
    ("lies beyond its letter buffer", lambda t: t["p_inss"]["seq_off"].__setitem__(slice(None), (1 << 64) - 3)),
    ("slot after is named by two nodes", lambda t: t["applied"]["nodes"].__setitem__(1, t["applied"]["nodes"][1][:3] + t["applied"]["nodes"][0][3:5] + (0,))),
    ("slot after is named by no node", lambda t: t["applied"]["nodes"].pop()),
    ("names a slot outside its block", lambda t: t["applied"]["nodes"].__setitem__(0, t["applied"]["nodes"][0][:4] + (1000, 0))),
    ("names a slot outside its block", lambda t: t["applied"]["nodes"].__setitem__(0, t["applied"]["nodes"][0][:3] + (len(t["applied"]["blocks"]), 0, 0))),
]


@pytest.mark.parametrize("at", range(len(DEVICE_REFUSALS)))
def test_refused_on_the_device(gpu_lib, at):
    message, change = DEVICE_REFUSALS[at]
    with pytest.raises(batch.PgaError, match="pga_assemble_blocks: .*" + message):
        asm.assemble_blocks(_corrupt(sg.case("alternating"), change), dll=gpu_lib.dll)
    check(gpu_lib.dll, sg.case("alternating"))                                    # (and the next call is sound)


def test_null_lists_with_counts(gpu_lib):
    K = asm.Tables(sg.case("alternating")["t"])
    b, plan, sl, pr, ap_ = K.call_args()
    for bad in ((b[:3] + (None,) + b[4:], plan, sl, pr, ap_), (b, plan[:2] + (None,) + plan[3:], sl, pr, ap_), (b, plan, None, pr, ap_), (b, plan, sl, (None,) + pr[1:], ap_), (b, plan, sl, pr, None)):
        with pytest.raises(batch.PgaError, match="null argument"):
            asm.assemble_blocks_raw(*bad, dll=gpu_lib.dll, ins_seq_len=len(K.L))


# ---------------------------------------------------------------- 4. the empty cases
def test_empty_inputs(gpu_lib):
    got = asm.assemble_blocks({"blocks": [], "counts": [], "subs": [], "dels": [], "inss": [], "ins_seq": b""}, dll=gpu_lib.dll)
    assert got["totals"] == (0, 0, 0, 0, 0, 0) and got["who"] is None
    k = sg.case("no_cut")                                                       # an empty cut: the input copied, letters compacted, no who; no merged block
    got = asm.assemble_blocks(k["t"], dll=gpu_lib.dll)
    assert got["who"] is None and got["origin"] == [0, 1, 2] and got["counts"].tolist() == np.asarray(k["t"]["counts"]).tolist()
    assert sg.resolved(got) == sg.resolved({"inss": k["t"]["inss"]}, k["t"]["ins_seq"]) and got["inss"]["seq_off"].tolist() == (np.cumsum(got["inss"]["len"]) - got["inss"]["len"]).tolist()
    assert asm.assemble_blocks(k["t"], asm.MERGED_ONLY, dll=gpu_lib.dll)["totals"] == (0, 0, 0, 0, 0, 0)


def test_last_ms_reports_the_three_phases(gpu_lib):
    asm.assemble_blocks(sg.case("one_heavy")["t"], dll=gpu_lib.dll)
    ms = asm.last_ms(gpu_lib.dll)
    assert len(ms) == 3 and all(0 < x < 5000 for x in ms), ms


# ---------------------------------------------------------------- 5. the output goes on by pointer: pga_detach_unaligned
def _valid(rng, idx):
    """edits that hold on every block of the case (the shortest has 5 letters); every third result spells its member without an aligned
    position on the merged block (20 letters): an orphan"""
    e = sg._edit(rng, 2, 1, 2, ins_lens=np.array([3, 7]))
    e[0]["pos"], e[1]["pos"], e[1]["len"], e[2]["pos"] = [0, 3], 1, 2, [2, 5]
    return e


def _valid_result(rng, rank):
    if rank % 3:
        return _valid(rng, rank)
    e = sg._edit(rng, 0, 1, 1, ins_lens=np.array([12 + rank]))
    e[1]["pos"], e[1]["len"], e[2]["pos"] = 0, 20, 0
    return e


def test_merged_blocks_go_to_detach_by_pointer(gpu_lib):
    dll = gpu_lib.dll
    k = sg.build(ag.case("interleaved_merge"), 77, before=_valid, sliced=_valid, result=_valid_result)
    K = asm.Tables(k["t"])
    out = asm.assemble_blocks_raw(*K.call_args(), flags=asm.MERGED_ONLY, dll=dll, keep=K, ins_seq_len=len(K.L))
    try:
        assert sg.same(out.to_arrays(), k["exp"][asm.MERGED_ONLY]) is None
        letters = C.string_at(out.out.ins_seq, out.out.n_ins_letters)
        d = dt.detach_unaligned_raw(out.block_args(), out.who, dll)              # pointers into the output, nothing repacked
        try:
            got = (d.to_dicts(letters), [{f: v for f, v in o.items() if f != "cons_off"} for o in d.orphans()], d.member_map())
        finally:
            d.free()
    finally:
        out.free()
    arrays = dt.merged_blocks(*sg.merged_blocks_input(k))
    args, keep = dt.arrays_args(arrays)
    d = dt.detach_unaligned_raw(args, k["exp"][asm.MERGED_ONLY]["who"], dll, keep=keep)
    try:
        want = (d.to_dicts(keep.L), [{f: v for f, v in o.items() if f != "cons_off"} for o in d.orphans()], d.member_map())
    finally:
        d.free()
    assert got == want and len(got[1]) == 2 and all(o["status"] == 0 for o in got[1]) and sorted(o["len"] for o in got[1]) == [12, 15]


# ---------------------------------------------------------------- 6. a whole round chained by pointer against the round in dicts
def _canon(g):
    """a graph with every edit list as a list of tuples"""
    edit = lambda e: {f: [tuple(x) for x in e[f]] for f in ("subs", "dels", "inss")}
    return {"paths": {p: dict(v, nodes=list(v["nodes"])) for p, v in g["paths"].items()}, "nodes": {n: dict(v, position=tuple(v["position"])) for n, v in g["nodes"].items()},
            "blocks": {b: {"consensus": v["consensus"], "alignments": {n: edit(e) for n, e in v["alignments"].items()}} for b, v in g["blocks"].items()}}


def _round(run):
    try:
        return _canon(run())
    except asm.MergeError:
        return "MergeError"


def _path_sequences(dll, block_args, lists, expected=None):
    """pga_reconstruct on block arrays given by pointer and the (blocks, paths, nodes) lists of the flat graph that goes with them (node
    (block, member) is global member first_member[block] + member); every path unrotated.  expected None: -> the sequence of every path;
    otherwise verify mode against those sequences -> [(status, n_mismatch)]"""
    from pangraph_amd.reconstruct import _bind as bind_recon, recon_node_t, recon_path_t, recon_res_t
    from pangraph_amd.reconsensus import rc_block_t
    _ptr = asm._ptr
    bind_recon(dll)
    blocks, paths, nodes = lists
    B = C.cast(block_args[1], C.POINTER(rc_block_t))
    first = [0]
    for i in range(block_args[0]):
        first.append(first[-1] + B[i].n_members)
    n = max(len(paths), 1)
    P, N, R = (recon_path_t * n)(), (recon_node_t * max(len(nodes), 1))(), (recon_res_t * n)()
    for k, x in enumerate(nodes):
        N[k].member, N[k].reverse = first[x[3]] + x[4], x[5]
    for i, p in enumerate(paths):
        P[i].n_nodes = p[2]
    call = lambda exp_p, exp_n, out: dll.pga_reconstruct(block_args[0], *[_ptr(a) for a in block_args[1:7]], len(paths), P, N, exp_p, exp_n, R, out)
    if expected is not None:
        keep = [bytes(s) for s in expected]
        for i, s in enumerate(keep):
            P[i].tot_len = len(s)
        if call((C.c_char_p * n)(*keep), (C.c_uint64 * n)(*[len(s) for s in keep]), None) != 0:
            raise batch.PgaError(dll.pga_last_error().decode())
        return [(R[i].status, R[i].n_mismatch) for i in range(len(paths))]
    out = C.POINTER(C.c_char)()
    for attempt in range(2):                                                     # the first call only measures: res[].len is always the built length
        if out:
            dll.pga_free(C.cast(out, C.c_void_p))
        if call(None, None, C.byref(out)) != 0:
            raise batch.PgaError(dll.pga_last_error().decode())
        for i in range(len(paths)):
            P[i].tot_len = R[i].len
    try:
        assert all(R[i].status == 0 for i in range(len(paths))), [R[i].status for i in range(len(paths))]
        return [C.string_at(C.addressof(out.contents) + R[i].seq_off, R[i].len) if R[i].len else b"" for i in range(len(paths))]
    finally:
        if out:
            dll.pga_free(C.cast(out, C.c_void_p))


def test_merge_round_on_the_device_against_the_round_in_dicts(gpu_lib, oracle_lib):
    import promise_ref as pr
    from pangraph_amd import topology as tp
    dll = gpu_lib.dll
    solve = lambda promises: [pr.solve_promise(oracle_lib.dll, q) for q in promises]
    verified = []

    def verify(K, graph_args, out, applied):
        """build_run.rs:141-148 on the live arrays: pga_reconstruct takes the assembled blocks and applied's graph by pointer, in verify mode
        against the sequences the paths spelled before"""
        before = _path_sequences(dll, K.args()[:7], tp.unpack_lists(graph_args))
        verified.append(_path_sequences(dll, out.block_args(), tp.unpack_lists(applied.graph_args()), before))

    def device(g, ms, thr):
        return asm._device_round(g, ms, thr, dll, tap=verify)

    thr = VEC["reweave"]["thr_len"]
    g0, matches = rg.reference_graph(VEC)
    g1, _ = rg.reference_graph(VEC)
    want = _round(lambda: asm.merge_round(g0, matches, thr, solve, dll=dll))
    assert _round(lambda: asm.merge_round(rg.reference_graph(VEC)[0], matches, thr, blocks="device", dll=dll)) == want
    got = _round(lambda: device(g1, matches, thr))
    assert got == want and want != "MergeError" and sum(1 for b in want["blocks"] if b not in rg.reference_graph(VEC)[0]["blocks"]) == 6
    n_done = n_members = 0
    for seed in range(40):                                                       # (random letters under random CIGARs: most rounds end in solve_promise's Err, on both sides)
        g, ms = ag.random_graph(seed)
        want = _round(lambda: asm.merge_round(ag.random_graph(seed)[0], ms, rg.THR, solve, dll=dll))
        got = _round(lambda: device(g, ms, rg.THR))
        assert got == want, seed
        if want != "MergeError":
            n_done += 1
            n_members += sum(len(v["alignments"]) for v in want["blocks"].values())
    assert n_done >= 6 and n_members >= 60, (n_done, n_members)
    assert len(verified) == 1 + n_done and all(v == (0, 0) for per in verified for v in per) and sum(len(per) for per in verified) >= 10


# ---------------------------------------------------------------- 7. two rounds: round 2's graph before is round 1's output, by pointer
def test_two_rounds_chained_by_pointer(gpu_lib):
    dll = gpu_lib.dll
    for name, seed in (("reference", 0), ("interleaved_merge", 1)):
        c = ag.case(name)
        nxt = ag.fresh_cut(c, seed)                                              # some of the blocks round 1 made, cut again
        assert nxt is not None and nxt["args"][3]
        k1 = sg.build(c, 40 + seed)
        e1 = k1["exp"][0]
        off = np.zeros((len(e1["counts"]) + 1, 3), np.int64)
        off[1:] = np.cumsum(e1["counts"].astype(np.int64), axis=0)
        member = lambda rng, i: tuple(e1[f][off[i, q]:off[i + 1, q]].copy() for q, f in enumerate(("subs", "dels", "inss")))     # round 1's members are round 2's
        k2 = sg.build(nxt, 50 + seed, before=member, pool0=e1["ins_seq"])
        assert k2["t"]["counts"].tolist() == e1["counts"].tolist() and [b[1] for b in k2["t"]["blocks"]] == [b[1] for b in e1["blocks"]]
        K1, K2 = asm.Tables(k1["t"]), asm.Tables(k2["t"])
        first = asm.assemble_blocks_raw(*K1.call_args(), dll=dll, keep=K1, ins_seq_len=len(K1.L))
        try:
            assert sg.same(first.to_arrays(), e1) is None
            _, plan, sliced, promised, applied = K2.call_args()
            second = asm.assemble_blocks_raw(first.block_args(), plan, sliced, promised, applied, dll=dll, keep=K2, ins_seq_len=first.out.n_ins_letters)
            try:
                got = second.to_arrays()
                assert sg.same(got, k2["exp"][0]) is None, (name, sg.same(got, k2["exp"][0]))
                assert any(o >= 0 for o in got["origin"]) and any(o < 0 for o in got["origin"])
            finally:
                second.free()
        finally:
            first.free()


# ---------------------------------------------------------------- 8. one round of simplify on the output: pga_plan_simplify + pga_merge_blocks
def _valid10(rng, idx):
    """edits that hold on blocks of 8 letters and more"""
    e = sg._edit(rng, 2, 1, 2, ins_lens=np.array([3, 7]))
    e[0]["pos"], e[1]["pos"], e[1]["len"], e[2]["pos"] = [0, 3], 6, 2, [4, 5]
    return e


def test_output_goes_to_plan_simplify_and_merge_blocks(gpu_lib):
    from pangraph_amd import simplify as sp
    from pangraph_amd import topology as tp
    from pangraph_amd.reconstruct import _Packed
    dll = gpu_lib.dll
    c = ag.case("forty_intervals")                                               # forty pieces of one block, in a row on every path: transitive edges
    k = sg.build(c, 88, before=_valid10, sliced=_valid10)
    K = asm.Tables(k["t"])
    graph = tp.pack_lists(*[c["exp"][f] for f in ("blocks", "paths", "nodes")])   # the graph of the same round (what pga_apply_merge returns)
    plan = tp.plan_round_raw(graph, dll=dll, keep=graph)
    try:
        edges, partner = [r["merge"] for r in plan.round()], list(plan.partner())
    finally:
        plan.free()
    assert len(edges) >= 10
    out = asm.assemble_blocks_raw(*K.call_args(), dll=dll, keep=K, ins_seq_len=len(K.L))
    try:
        assert sg.same(out.to_arrays(), k["exp"][0]) is None
        m = sp.merge_blocks_raw(out.block_args(), edges, partner, dll)           # pointers into the output
        try:
            got = m.to_dicts()
        finally:
            m.free()
    finally:
        out.free()
    K2 = _Packed(sg.dicts_of(k["exp"][0]), [])                                  # the same blocks, packed from the expectation
    m = sp.merge_blocks_raw(K2.args()[:7], edges, partner, dll, keep=K2)
    try:
        want = m.to_dicts()
    finally:
        m.free()
    assert got == want and all(e["status"] == 0 for e in got) and all(len(e["members"]) == 3 for e in got)
