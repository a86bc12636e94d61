"""pga_detach_unaligned (pga_detach.hip: detach_unaligned_nodes on the device) and pangraph_amd.detach against the restatement
tests/detach_ref.py and the reference's own unit-test values (tests/golden/detach_vectors.json).  Every comparison is exact."""
import copy
import ctypes as C
import gzip
import json
import os

import pytest

import detach_gen as dg
import detach_ref as dr
import mapvarbind as mb
import reconstruct_ref as rr
import simplify_gen as sg
import simplify_ref as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import detach as dt  # noqa: E402
from pangraph_amd.mapvar import params  # noqa: E402
from pangraph_amd.reconsensus import _edit, rc_out_t  # noqa: E402
from pangraph_amd.reconstruct import _Packed, reconstruct  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "detach_vectors.json")))


def check_batch(dll, blocks, who):
    """the product against the restatement: every block, member list, map entry and orphan record; the letters and the id of an orphan with
    status 0 (the others keep their slot and their length)"""
    got = dt.detach_unaligned(blocks, who, dll=dll)
    exp = dr.expected_call(blocks, who)
    assert got["member_map"] == exp["member_map"]
    assert len(got["orphans"]) == len(exp["orphans"]) and len(got["blocks"]) == len(exp["blocks"]) == len(blocks) + len(exp["orphans"])
    at = 0
    for k, (g, e) in enumerate(zip(got["orphans"], exp["orphans"])):
        assert {f: g[f] for f in ("member", "node_id", "block", "len", "status")} == {f: e[f] for f in ("member", "node_id", "block", "len", "status")}, (k, g, e)
        assert g["cons_off"] % 16 == 0 and g["cons_off"] >= at, (k, g)             # counts and offsets do not depend on a status
        at = g["cons_off"] + g["len"]
        if e["status"] == 0:
            assert g["seq"] == e["seq"] and g["block_id"] == e["block_id"], (k, g, e)
        else:
            assert g["block_id"] == 0
    for i, (g, e) in enumerate(zip(got["blocks"], exp["blocks"])):
        if e["consensus"] is not None:
            assert g["consensus"] == e["consensus"], i
        assert g["members"] == e["members"], i
    return got


# ---------------------------------------------------------------- 1. the reference's own values
def test_reference_vectors(gpu_lib):
    dll = gpu_lib.dll
    for case in ("forward", "reverse"):                                          # create_new_node_and_block: a member that is its whole sequence
        v = VEC["create_new_node_and_block"][case]
        blocks = [{"consensus": "", "members": [{"subs": [], "dels": [], "inss": [(0, v["seq"])]}]}]
        got = check_batch(dll, blocks, [[(v["node_id"], v["old_node"]["strand"] == "-")]])
        (o,) = got["orphans"]
        assert o["seq"] == v["expected_consensus"] and o["status"] == 0 and o["block_id"] == dr.block_id(v["node_id"], v["expected_consensus"])
        assert got["blocks"] == [{"consensus": "", "members": []}, {"consensus": v["expected_consensus"], "members": [{"subs": [], "dels": [], "inss": []}]}]
    v = VEC["extract_unaligned_nodes_simple"]
    blk = sr.from_json({"paths": {}, "nodes": {}, "blocks": {"0": v["block"]}})["blocks"][0]
    ids = sorted(blk["alignments"])
    got = check_batch(dll, [{"consensus": blk["consensus"], "members": [blk["alignments"][n] for n in ids]}], [[(n, False) for n in ids]])
    assert [(o["node_id"], o["seq"]) for o in got["orphans"]] == [(u["node_id"], u["sequence"]) for u in v["expected_unaligned"]]
    want = sr.from_json({"paths": {}, "nodes": {}, "blocks": {"0": v["expected_block"]}})["blocks"][0]
    assert got["blocks"][0] == {"consensus": want["consensus"], "members": [want["alignments"][n] for n in sorted(want["alignments"])]} and got["member_map"] == [0, 1]
    v = VEC["detach_unaligned_nodes"]
    g = dt.detach_graph(dt.normalize(v["graph"]), [0], dll=dll)
    new = v["expected_new_block"]
    new_id = dr.block_id(new["node_id"], new["consensus"])
    assert len(g["blocks"]) == v["expected_n_blocks"]
    assert g["blocks"][0] == sr.from_json({"paths": {}, "nodes": {}, "blocks": {"0": v["expected_block_0"]}})["blocks"][0]
    assert g["blocks"][new_id] == {"consensus": new["consensus"], "alignments": {new["node_id"]: {"subs": [], "dels": [], "inss": []}}}
    assert g["nodes"] == {int(k): {"block_id": new_id if n["block_id"] == "@new" else n["block_id"], "path_id": n["path_id"], "strand": n["strand"], "position": tuple(n["position"])}
                          for k, n in v["expected_nodes"].items()}


# ---------------------------------------------------------------- 2. the smallest shapes at which the kernels can go wrong
def test_edge_case_batch(gpu_lib):
    got = check_batch(gpu_lib.dll, *dg.edge_batch())
    assert all(o["status"] == 0 for o in got["orphans"]) and {o["len"] for o in got["orphans"]} >= set(dg.ORPHAN_LENGTHS)


# ---------------------------------------------------------------- 3. random batches
@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_batches(gpu_lib, seeds):
    for seed in seeds:
        check_batch(gpu_lib.dll, *dg.random_batch(seed))


# ---------------------------------------------------------------- 4. statuses
def test_rejected_orphans_next_to_a_good_one(gpu_lib):
    blocks, who = dg.status_batch()
    got = check_batch(gpu_lib.dll, blocks, who)
    assert [o["status"] for o in got["orphans"]] == [2, 3, 0, 0, 3]
    good = got["orphans"][2]
    assert good["seq"] == "TGCAACGT" and good["block_id"] == dr.block_id(good["node_id"], "TGCAACGT")
    # every count and offset is what it is when the letters are ordinary ones
    clean = copy.deepcopy(blocks)
    clean[0]["members"][0]["inss"] = [(0, "ACGTACGT")]; clean[0]["members"][1]["inss"] = [(24, "ACGAT")]; clean[1]["members"][1]["subs"] = [(10, "A")]
    ref = check_batch(gpu_lib.dll, clean, who)
    assert all(o["status"] == 0 for o in ref["orphans"])
    layout = lambda r: ([(o["member"], o["block"], o["len"], o["cons_off"]) for o in r["orphans"]], r["member_map"], [len(b["members"]) for b in r["blocks"]])
    assert layout(got) == layout(ref)


# ---------------------------------------------------------------- 5. malformed input
def test_malformed_input_fails_the_call_and_leaves_the_library_usable(gpu_lib):
    dll = gpu_lib.dll
    blocks = [{"consensus": "ACGTACGT", "members": [{"subs": [(1, "A")], "dels": [(2, 2)], "inss": [(8, "AC")]}, {"subs": [], "dels": [(0, 8)], "inss": [(0, "GG")]}]},
              {"consensus": "TTGCA", "members": [{"subs": [], "dels": [], "inss": [(0, "G")]}]}]
    who = [[(5, False), (9, True)], [(11, True)]]

    def fails(blocks, needle):
        with pytest.raises(batch.PgaError, match=needle):
            dt.detach_unaligned(blocks, who, dll=dll)
        check_batch(dll, blocks_ok, who)                                          # the next call works

    blocks_ok = blocks
    for field, entry, needle in (("subs", (8, "A"), "substitution beyond"), ("dels", (7, 2), "deletion beyond"), ("inss", (9, "A"), "insertion beyond")):
        broken = copy.deepcopy(blocks)
        broken[0]["members"][0][field].append(entry)
        fails(broken, needle)
    K = _Packed(blocks, [])
    args = list(K.args()[:7])
    flat = [w for blk in who for w in blk]
    with pytest.raises(batch.PgaError, match="null node list"):
        dt.detach_unaligned_raw(args, None, dll)
    a = list(args)
    a[6] = None                                                                   # NULL insertion letters with a length
    with pytest.raises(batch.PgaError, match="null insertion letters"):
        dt.detach_unaligned_raw(a, flat, dll)
    for null_at in (1, 2, 3, 4, 5):
        a = list(args)
        a[null_at] = None
        with pytest.raises(batch.PgaError):
            dt.detach_unaligned_raw(a, flat, dll)
    out = dt.detach_unaligned_raw([0] + args[1:], [], dll)                        # no block: empty lists, no device call
    assert (out.n_blocks, out.n_orphans) == (0, 0) and not out.out.cons and not out.out.orphans
    out.free()
    check_batch(dll, blocks, who)


# ---------------------------------------------------------------- 6. the next entry reads the output in place
def _reconsensus_raw(dll, graph_args, n_members):
    """pga_reconsensus over arrays that exist already -> per block (kind, consensus, member edits, majority edit, member statuses)"""
    out, p = rc_out_t(), params()
    dll.pga_reconsensus.restype = C.c_int
    dll.pga_reconsensus.argtypes = [C.c_int64] + [C.c_void_p] * 8
    dll.pga_rc_free.argtypes = [C.c_void_p]
    assert dll.pga_reconsensus(*graph_args, C.byref(p), C.byref(out)) == 0
    res, m = [], 0
    try:
        cbase = C.addressof(out.cons.contents)
        for i, n in enumerate(n_members):
            r = out.blocks[i]
            maj = _edit(out.m_subs, out.m_dels, out.m_inss, out.m_ins_seq, (r.sub_off, r.n_subs), (r.del_off, r.n_dels), (r.ins_off, r.n_inss))
            mem, status = [], []
            for _ in range(n):
                v = out.members[m]
                mem.append(_edit(out.subs, out.dels, out.inss, out.ins_seq, (v.sub_off, v.n_subs), (v.del_off, v.n_dels), (v.ins_off, v.n_inss)))
                status.append(v.status)
                m += 1
            res.append((r.kind, C.string_at(cbase + r.cons_off, r.cons_len).decode(), mem, maj, status))
    finally:
        dll.pga_rc_free(C.byref(out))
    return res


def test_reconsensus_reads_the_output_by_pointer(gpu_lib):
    dll = gpu_lib.dll
    import random
    rng = random.Random(11)
    blocks, who = [], []
    for b, L in enumerate((120, 90, 200)):
        cons = "".join(rng.choice("ACGT") for _ in range(L))
        members = []
        for k in range(5):
            members.append({"subs": [(rng.randrange(L), rng.choice("ACGT")) for _ in range(3)], "dels": [(10 * k + 5, 3)], "inss": [(rng.randrange(L + 1), "ACGTA"[:1 + k])]})
        members[b] = {"subs": [], "dels": [(0, L // 2), (L // 2, L - L // 2)], "inss": [(L // 2, "".join(rng.choice("ACGT") for _ in range(30 + b)))]}      # one orphan per block, at another place each
        blocks.append({"consensus": cons, "members": members})
        who.append([(100 * b + k + 1, k % 2 == 1) for k in range(5)])
    exp = dr.expected_call(blocks, who)
    assert len(exp["orphans"]) == 3 and all(o["status"] == 0 and o["len"] for o in exp["orphans"])
    K = _Packed(blocks, [])
    out = dt.detach_unaligned_raw(K.args()[:7], [w for blk in who for w in blk], dll, keep=K)
    try:
        assert out.to_dicts(K.L) == exp["blocks"]
        got = _reconsensus_raw(dll, out.graph_args(K.L), out.n_members())          # pointers into the output, the caller's insertion letters
    finally:
        out.free()
    K2 = _Packed(exp["blocks"], [])                                                # the same blocks, packed from the restatement's result
    want = _reconsensus_raw(dll, K2.args()[:7], [len(b["members"]) for b in exp["blocks"]])
    assert got == want and len(got) == 6 and [len(r[2]) for r in got] == [4, 4, 4, 1, 1, 1]


# ---------------------------------------------------------------- 7. end to end on the plasmid graph
def test_plasmids_detached_nodes_reconstruct(gpu_lib):
    """about 20 nodes spelled without an aligned position (Del(0, cons_len) + Ins(0, the member's own sequence)): detach_graph gives each a
    block of its own, and every path still reconstructs to its genome.  Does not lean on the restatement of detach_unaligned.rs."""
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    genome = dict(zip(*rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))))
    g = dt.normalize(G)
    assert len(g["paths"]) == 15
    reverse = [n for n in sorted(g["nodes"]) if g["nodes"][n]["strand"] == "-"]
    forward = [n for n in sorted(g["nodes"]) if g["nodes"][n]["strand"] == "+"]
    assert len(reverse) == 33
    chosen = reverse[:8] + forward[:12]
    assert len(chosen) == 20
    touched = set()
    for n in chosen:
        blk = g["blocks"][g["nodes"][n]["block_id"]]
        seq = mb.apply_edit(blk["consensus"], blk["alignments"][n])
        assert seq
        blk["alignments"][n] = {"subs": [], "dels": [(0, len(blk["consensus"]))], "inss": [(0, seq)]}
        touched.add(g["nodes"][n]["block_id"])
    before = copy.deepcopy(g)
    dt.detach_graph(g, sorted(touched), dll=gpu_lib.dll)
    assert len(g["blocks"]) == len(before["blocks"]) + len(chosen)
    for n in chosen:
        node, old = g["nodes"][n], before["nodes"][n]
        assert node["strand"] == "+" and node["position"] == old["position"] and node["path_id"] == old["path_id"] and node["block_id"] != old["block_id"]
        assert list(g["blocks"][node["block_id"]]["alignments"]) == [n] and n not in g["blocks"][old["block_id"]]["alignments"]
    assert {n: v for n, v in g["nodes"].items() if n not in chosen} == {n: v for n, v in before["nodes"].items() if n not in chosen}
    blocks, paths, names = sg.recon_input(g)
    res = reconstruct(blocks, paths, [genome[n] for n in names], want_seqs=False, dll=gpu_lib.dll)
    assert [(r["status"], r["n_mismatch"]) for r in res] == [(0, 0)] * 15


# ---------------------------------------------------------------- 8. nothing to detach
def test_no_orphans_returns_the_input(gpu_lib):
    blocks, who = dg.edge_batch()
    blocks = [{"consensus": b["consensus"], "members": [e for e in b["members"] if dr.aligned_count(e, len(b["consensus"])) != 0]} for b in blocks]
    who = [[(7 + k, bool(k & 1)) for k in range(len(b["members"]))] for b in blocks]
    assert sum(len(b["members"]) for b in blocks) > 10
    K = _Packed(blocks, [])
    out = dt.detach_unaligned_raw(K.args()[:7], [w for blk in who for w in blk], gpu_lib.dll, keep=K)
    try:
        assert out.n_orphans == 0 and out.n_blocks == len(blocks) and not out.out.cons and not out.out.orphans
        assert out.to_dicts(K.L, with_offsets=True) == [{"consensus": b["consensus"], "members": [dict(e, seq_off=so) for e, so in zip(b["members"], offs)]}
                                                         for b, offs in zip(blocks, _seq_offs(K, blocks))]
        assert out.member_map() == list(range(K.n_mem))
    finally:
        out.free()


def _seq_offs(K, blocks):
    """per block, per member: the seq_off of its insertions in the packed input"""
    res, i = [], 0
    for b in blocks:
        row = []
        for e in b["members"]:
            row.append([K.I[i + k].seq_off for k in range(len(e["inss"]))])
            i += len(e["inss"])
        res.append(row)
    return res
