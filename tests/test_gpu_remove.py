"""pga_remove_paths (pga_remove.hip: the path removal of `pangraph simplify` on the device) against tests/remove_gen.py's host_remove --
pangraph_amd.simplify.remove_path applied path by path -- on every named case and on seeded random graphs, with and without
PGA_REMOVE_COMPACT_LETTERS; its output by pointer into pga_plan_simplify and pga_reconstruct; simplify(paths="device") on the plasmids; and
every malformed input.  Every comparison is exact.  What each case holds is pinned by tests/test_remove_cpu.py."""
import copy
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import reconstruct_ref as rr
import remove_gen as rg
import simplify_ref as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import remove as rm  # noqa: E402
from pangraph_amd import simplify as sp  # noqa: E402
from pangraph_amd import topology as tp  # noqa: E402
from pangraph_amd.reconstruct import recon_node_t, recon_path_t, reconstruct_packed  # noqa: E402

FLAGS = (0, rm.COMPACT_LETTERS)


def call(case, flags, dll):
    args, block_args, n_letters, K = rg.pack(case)
    return rm.remove_paths_raw(args, block_args, case["keep"], flags, n_letters, dll, keep_alive=K)


def check(case, dll, expected=None):
    for flags in FLAGS:
        exp = expected[flags] if expected else rg.host_remove(case, flags)
        out = call(case, flags, dll)
        try:
            got = dict(out.to_lists(), dicts=out.to_dicts())
        finally:
            out.free()
        assert sorted(got) == sorted(rg.OUT_FIELDS)
        for f in rg.OUT_FIELDS:
            assert got[f] == exp[f], (flags, f)


# ---------------------------------------------------------------- 1. every named case, the random graphs, the graph past the second level
@pytest.mark.parametrize("name", sorted(rg.CASES))
def test_named_case(gpu_lib, name):
    check(rg.case(name), gpu_lib.dll, {f: rg.expected(name, f) for f in FLAGS})


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_graphs(gpu_lib, seeds):
    for seed in seeds:
        check(rg.random_case(seed), gpu_lib.dll)


def _view(ptr, dtype, n):
    return np.frombuffer((C.c_char * (n * dtype.itemsize)).from_address(C.cast(ptr, C.c_void_p).value), dtype, n) if n else np.zeros(0, dtype)


@pytest.mark.parametrize("flags", FLAGS)
def test_past_the_second_level_of_the_tile_scan(gpu_lib, flags):
    inp, exp = rg.second_level()
    ptr = lambda a: C.c_void_p(a.ctypes.data)
    args = (len(inp["blocks"]), ptr(inp["blocks"]), len(inp["paths"]), ptr(inp["paths"]), len(inp["nodes"]), ptr(inp["nodes"]))
    block_args = (len(inp["blocks"]), ptr(inp["rc_blocks"]), ptr(inp["members"]), ptr(inp["subs"]), ptr(inp["dels"]), ptr(inp["inss"]), ptr(inp["ins_seq"]))
    out = rm.remove_paths_raw(args, block_args, (C.c_uint8 * 5)(*inp["keep"].tolist()), flags, len(inp["ins_seq"]), gpu_lib.dll, keep_alive=inp)
    try:
        o = out.out
        assert (o.n_blocks, o.n_paths, o.n_nodes, o.n_members, o.n_dead_blocks) == (4, 3, len(exp["nodes"]), int(exp["kept"].sum()), 0)
        assert (o.n_subs, o.n_dels, o.n_inss, o.n_ins_letters) == (len(exp["subs"]), len(exp["dels"]), len(exp["inss"]), len(exp["ins_seq"]) if flags else 0)
        for field, dtype, want in (("blocks", rg.NP_BLOCK, exp["blocks"]), ("paths", rg.NP_PATH, exp["paths"]), ("nodes", rg.NP_NODE, exp["nodes"]), ("rc_blocks", rg.NP_RC, exp["rc_blocks"]),
                                   ("members", rg.NP_MEMBER, exp["members"]), ("subs", rg.NP_SUB, exp["subs"]), ("dels", rg.NP_DEL, exp["dels"]),
                                   ("inss", rg.NP_INS, exp["inss_compact"] if flags else exp["inss"])):
            got = _view(getattr(o, field), dtype, len(want))
            assert got.tobytes() == want.tobytes(), field
        assert np.array_equal(_view(o.member_map, np.dtype(np.int64), len(exp["kept"])), exp["member_map"]) and np.array_equal(_view(o.path_map, np.dtype(np.int32), 5), exp["path_map"])
        if flags:
            assert _view(o.ins_seq, np.dtype(np.uint8), len(exp["ins_seq"])).tobytes() == exp["ins_seq"].tobytes()
        else:
            assert not o.ins_seq
    finally:
        out.free()


# ---------------------------------------------------------------- 2. the output by pointer into the next calls
def _transitive_by_index(g, bids):
    at = {b: i for i, b in enumerate(bids)}
    return [(at[b1], at[b2], "+-".index(s1), "+-".index(s2)) for (b1, s1), (b2, s2) in sp.find_transitive_edges(g)]


def test_output_is_the_input_of_plan_simplify(gpu_lib):
    n_edges = 0
    for case in [rg.case(n) for n in ("reference", "dies", "wrap_node", "dead_before", "one_block_twice", f"tile_{rg.TILE}")] + [rg.random_case(s) for s in range(12)]:
        g = rg.graph_after(case)
        out = call(case, 0, gpu_lib.dll)
        try:
            plan = tp.plan_round_raw(out.graph_args(), flags=tp.EDGES_ONLY, dll=gpu_lib.dll)
            try:
                got = [e[:4] for e in plan.transitive()]
            finally:
                plan.free()
        finally:
            out.free()
        assert got == _transitive_by_index(g, [b[0] for b in case["lists"][0]])
        n_edges += len(got)
    assert n_edges >= 5


@pytest.fixture(scope="module")
def plasmids():
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    names = [G["paths"][k]["name"] for k in sorted(G["paths"], key=int)]
    return G, names, dict(zip(*rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))))


@pytest.mark.parametrize("n_paths", [1, 3, 8])
def test_output_is_the_input_of_reconstruct(gpu_lib, plasmids, n_paths):
    G, names, genome = plasmids
    g = sp.normalize(G)
    focal = set(names[:n_paths])
    R = rm.removed_graph(g, focal, "device", gpu_lib.dll)
    try:
        out = R.out
        lists = out.to_lists()
        want = copy.deepcopy(g)
        for pid in [pid for pid in sorted(want["paths"]) if want["paths"][pid]["name"] not in focal]:
            sp.remove_path(want, pid)
        assert R.g == want and lists["counts"][4] == len(g["blocks"]) - len(want["blocks"]) > 0
        first = [0]
        for _, n in lists["rc_blocks"]:
            first.append(first[-1] + n)
        kept = [want["paths"][p[0]] for p in lists["paths"]]

        class View:
            n_paths = len(kept)
            P = (recon_path_t * len(kept))(*[recon_path_t(k["tot_len"], lists["nodes"][p[1]][1] if p[2] else 0, p[2], 0) for k, p in zip(kept, lists["paths"])])
            N = (recon_node_t * len(lists["nodes"]))(*[recon_node_t(first[n[3]] + n[4], n[5], 0) for n in lists["nodes"]])

            def args(self):
                return out.block_args() + (self.n_paths, self.P, self.N)

        res = reconstruct_packed(View(), [genome[k["name"]] for k in kept], want_seqs=False, dll=gpu_lib.dll)
        assert [(r["status"], r["n_mismatch"]) for r in res] == [(0, 0)] * n_paths
    finally:
        R.close()


@pytest.mark.parametrize("n_paths", [1, 3, 8])
def test_simplify_with_the_paths_removed_on_the_device(gpu_lib, plasmids, n_paths):
    G, names, _ = plasmids
    focal = names[:n_paths]
    for topology in (None, "device"):
        trace = {}
        g = sp.simplify(G, focal, dll=gpu_lib.dll, trace=trace, topology=topology, paths="device")
        assert g == sr.simplify(sr.from_json(G), set(focal), trace["rounds"])
        assert trace["zero_copy"][0] is True and len(trace["zero_copy"]) == len(trace["rounds"]) and not sp.find_transitive_edges(g)
    assert rm.remove_paths(G, focal, dll=gpu_lib.dll) == rm.remove_paths(G, focal, dll=gpu_lib.dll, flags=rm.COMPACT_LETTERS)


# ---------------------------------------------------------------- 3. malformed input
def test_malformed_input_fails_the_call_and_leaves_the_library_usable(gpu_lib):
    dll = gpu_lib.dll
    base = rg.case("dead_before")                                            # blocks A, a dead entry, B, C; paths A+ B+ C+ | A+ C- | B- B+

    def fails(needle, flags=0, lists=None, edit=None, keep=base["keep"], null=None, n_letters=None, dicts=None):
        case = dict(base, lists=copy.deepcopy(lists or base["lists"]), dicts=dicts or base["dicts"])
        args, block_args, letters, K = rg.pack(case)
        if edit:
            edit(K)
        block_args = list(block_args)
        if null is not None:
            block_args[null] = None
        with pytest.raises(batch.PgaError, match=needle):
            rm.remove_paths_raw(args, tuple(block_args), keep, flags, letters if n_letters is None else n_letters, dll, keep_alive=K)
        check(rg.case("one_block_twice"), dll)                                # the next call works

    def nodes(k, **kw):
        b, p, n = copy.deepcopy(base["lists"])
        f = ("node_id", "pos0", "pos1", "block", "member", "reverse")
        n[k] = tuple(kw.get(x, v) for x, v in zip(f, n[k]))
        return b, p, n

    def paths(k, **kw):
        b, p, n = copy.deepcopy(base["lists"])
        f = ("path_id", "node_off", "n_nodes", "circular")
        p[k] = tuple(kw.get(x, v) for x, v in zip(f, p[k]))
        return b, p, n

    def blocks(k, **kw):
        b, p, n = copy.deepcopy(base["lists"])
        f = ("block_id", "cons_len", "depth", "alive")
        b[k] = tuple(kw.get(x, v) for x, v in zip(f, b[k]))
        return b, p, n

    # what pga_plan_simplify refuses on the host
    fails("member >= depth", lists=nodes(0, member=9))
    fails("block out of range", lists=nodes(0, block=4))
    fails("dead block", lists=nodes(0, block=1))
    fails("path ids are not ascending", lists=paths(1, path_id=1))
    fails("node_off is not the running sum", lists=paths(1, node_off=2))
    fails("do not sum to the node count", lists=paths(2, n_nodes=3))
    fails("not strictly ascending", lists=blocks(3, block_id=1))
    # this call's own
    fails("null keep", keep=None)
    fails("unknown flag", flags=2)
    fails("null argument", null=2)
    fails("null argument", null=3)
    fails("null argument", null=5)
    fails("differs from its depth", edit=lambda K: setattr(K.B[0], "n_members", 1))
    fails("dead block with members", edit=lambda K: setattr(K.B[1], "n_members", 1))
    # on the device: a slot named twice (and so another by none), a block deeper than its nodes
    fails("slot is named by", lists=nodes(3, member=0))
    deeper = copy.deepcopy(base["dicts"])
    deeper[0]["members"].append(copy.deepcopy(rg.tg.EDIT))
    fails("do not sum to its depth|slot is named by", lists=blocks(0, depth=3), dicts=deeper)
    # the letters: only with the flag, only for what is kept
    fails("null insertion letters", flags=rm.COMPACT_LETTERS, null=6)
    fails("beyond ins_seq_len", flags=rm.COMPACT_LETTERS, n_letters=1)
    fails("beyond ins_seq_len", flags=rm.COMPACT_LETTERS, edit=lambda K: [setattr(K.I[k], "seq_off", (1 << 64) - 1) for k in range(5)])
    args, block_args, letters, K = rg.pack(base)
    out = rm.remove_paths_raw(args, block_args[:6] + (None,), base["keep"], 0, 0, dll, keep_alive=K)           # without the flag the letters are not read
    try:
        assert out.to_lists()["inss"] == rg.expected("dead_before")["inss"] and not out.out.ins_seq
    finally:
        out.free()
    # no path at all: no device call, every block as it was or dead
    args = tp.pack_lists([(5, 9, 0, 0), (7, 4, 0, 0)], [], [])
    K = rg._Packed([{"consensus": "ACGTACGTA", "members": []}, {"consensus": "ACGT", "members": []}], [])
    out = rm.remove_paths_raw(args, K.args()[:7], [], 0, 0, dll, keep_alive=K)
    try:
        assert out.to_lists()["counts"] == (2, 0, 0, 0, 2, 0, 0, 0, 0) and out.to_lists()["blocks"] == [(5, 0, 0, 0), (7, 0, 0, 0)]
    finally:
        out.free()
    with pytest.raises(batch.PgaError, match="named by no node"):
        rm.remove_paths_raw(tp.pack_lists([(5, 9, 1, 1)], [], []), rg._Packed([{"consensus": "ACGTACGTA", "members": [dict(rg.tg.EDIT)]}], []).args()[:7], [], 0, 0, dll)
    check(base, dll)
