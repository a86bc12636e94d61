"""pga_merge_blocks (pga_merge.hip: the block concatenations of `pangraph simplify` on the device) and pangraph_amd.simplify against the
restatement tests/simplify_ref.py and the reference's own unit-test values (tests/golden/simplify_vectors.json).  Every comparison is
exact, list order inside every edit included."""
import copy
import ctypes as C
import gzip
import json
import os

import pytest

import reconstruct_ref as rr
import simplify_gen as sg
import simplify_ref as sr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd import batch  # noqa: E402
from pangraph_amd import simplify as sp  # noqa: E402
from pangraph_amd.reconstruct import _Packed, recon_node_t, recon_path_t, reconstruct, reconstruct_packed  # noqa: E402

VEC = json.load(open(os.path.join(GOLDEN, "simplify_vectors.json")))


def _block(b):
    """a block of the vectors -> {"consensus", "members"} in NodeId order"""
    blk = sr.from_json({"paths": {}, "nodes": {}, "blocks": {"0": b}})["blocks"][0]
    return {"consensus": blk["consensus"], "members": [blk["alignments"][n] for n in sorted(blk["alignments"])]}


def check_batch(dll, blocks, edges):
    """the product against the restatement: a status-0 edge exactly; a status-2 edge by its status and its counts"""
    got = sp.merge_blocks(blocks, edges, dll=dll)
    exp = sr.merge_batch(blocks, edges)
    assert len(got) == len(exp) == len(edges)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g["status"] == e["status"], (i, edges[i], g["status"], e["status"])
        if e["status"] == 0:
            assert g["consensus"] == e["consensus"], (i, edges[i])
            for k, (gm, em) in enumerate(zip(g["members"], e["members"])):
                assert gm == em, (i, k, edges[i], {f: (gm[f], em[f]) for f in gm if gm[f] != em[f]})
            assert len(g["members"]) == len(e["members"])
        else:
            counts, ins_lens = sr.merged_counts(blocks, edges[i])
            assert [(len(m["subs"]), len(m["dels"]), len(m["inss"])) for m in g["members"]] == counts
            assert [[len(s) for _, s in m["inss"]] for m in g["members"]] == ins_lens
            assert len(g["consensus"]) == len(blocks[edges[i]["left"]]["consensus"]) + len(blocks[edges[i]["right"]]["consensus"])
    return got


# ---------------------------------------------------------------- 1. the reference's own values
def test_reference_concatenations(gpu_lib):
    MB, SR = VEC["merge_blocks"], VEC["simplify_run"]
    blocks = [_block(MB["block_1"]), _block(MB["block_2"])]
    # a: block_1 ++ revcomp(block_2); b: revcomp(block_2) ++ block_1; c: block_1 ++ block_2 (the members pair up in NodeId order)
    edges = [{"left": 0, "right": 1, "left_rc": False, "right_rc": True, "partner": [0, 1, 2]}, {"left": 1, "right": 0, "left_rc": True, "right_rc": False, "partner": [0, 1, 2]},
             {"left": 0, "right": 1, "left_rc": False, "right_rc": False, "partner": [0, 1, 2]}]
    got = check_batch(gpu_lib.dll, blocks, edges)
    for case, g, order in (("a", got[0], "123"), ("b", got[1], "123"), ("c", got[2], "123")):
        want = MB[case]["expected_concat"]
        assert g["status"] == 0 and g["consensus"] == want["consensus"]
        for k, m in zip(order, g["members"]):
            w = want["alignments"]["@" + k]
            assert m == {"subs": [(x["pos"], x["alt"]) for x in w["subs"]], "dels": [(x["pos"], x["len"]) for x in w["dels"]], "inss": [(x["pos"], x["seq"]) for x in w["inss"]]}
    # block_ab through the whole command
    assert sp.simplify(SR["graph"], SR["focal"], dll=gpu_lib.dll) == sr.from_json(SR["expected_graph"])
    for case in "abc":
        v = MB[case]
        trace = {}
        g = sp.simplify(v["graph"], [None], dll=gpu_lib.dll, trace=trace)
        assert g == sr.simplify(sr.from_json(v["graph"]), {None}, trace["rounds"]) and len(trace["rounds"]) == 1


# ---------------------------------------------------------------- 2. sizes at which the kernels take another path
def test_edge_case_batch(gpu_lib):
    blocks, edges = sg.edge_batch()
    got = check_batch(gpu_lib.dll, blocks, edges)
    assert all(g["status"] == 0 for g in got)


@pytest.mark.parametrize("seeds", [range(0, 20), range(20, 40)])
def test_random_batches(gpu_lib, seeds):
    for seed in seeds:
        check_batch(gpu_lib.dll, *sg.random_batch(seed))


def test_status_2_edge_next_to_good_edges(gpu_lib):
    """a letter without a complement in one block: the edges that complement it report 2, every other edge is exact, and every count and
    offset is what it is when the letter is an ordinary one"""
    blocks, edges = sg.edge_batch()
    blocks = copy.deepcopy(blocks)
    bad = next(i for i, b in enumerate(blocks) if len(b["consensus"]) == 16)
    marked = copy.deepcopy(blocks)
    cons = marked[bad]["consensus"]
    marked[bad]["consensus"] = cons[:-1] + "x"
    marked[bad]["members"][0]["inss"][0] = (marked[bad]["members"][0]["inss"][0][0], "n" + marked[bad]["members"][0]["inss"][0][1][1:])
    exp = sr.merge_batch(marked, edges)
    hit = [i for i, e in enumerate(exp) if e["status"] == 2]
    assert hit and len(hit) < len(edges) and all(bad in (edges[i]["left"], edges[i]["right"]) for i in hit)
    check_batch(gpu_lib.dll, marked, edges)
    layouts = []
    for b in (blocks, marked):
        K = _Packed(b, [])
        out = sp.merge_blocks_raw(K.args()[:7], [(e["left"], e["right"], e["left_rc"], e["right_rc"]) for e in edges], [q for e in edges for q in e["partner"]], gpu_lib.dll, keep=K)
        try:
            d = out.to_dicts(with_offsets=True)
            layouts.append((out.member_off, out.counts(), [r["cons_off"] for r in d], [[m["seq_off"] for m in r["members"]] for r in d]))
        finally:
            out.free()
    assert layouts[0] == layouts[1]


# ---------------------------------------------------------------- 3. malformed input
def test_malformed_input_fails_the_call_and_leaves_the_library_usable(gpu_lib):
    blocks = [{"consensus": "ACGTACGT", "members": [{"subs": [(1, "A")], "dels": [(2, 2)], "inss": [(8, "AC")]}, {"subs": [], "dels": [], "inss": []}]},
              {"consensus": "TTGCA", "members": [{"subs": [], "dels": [], "inss": [(0, "G")]}, {"subs": [(4, "C")], "dels": [], "inss": []}]},
              {"consensus": "A", "members": [{"subs": [], "dels": [], "inss": []}]}]
    good = {"left": 0, "right": 1, "left_rc": False, "right_rc": True, "partner": [1, 0]}

    def fails(blocks, edges, needle):
        with pytest.raises(batch.PgaError, match=needle):
            sp.merge_blocks(blocks, edges, dll=gpu_lib.dll)
        check_batch(gpu_lib.dll, [copy.deepcopy(b) for b in blocks_ok], [good])          # the next call works

    blocks_ok = blocks
    fails(blocks, [dict(good, right=3)], "does not exist")
    fails(blocks, [dict(good, left=7)], "does not exist")
    fails(blocks, [dict(good, right=2, partner=[0, 0])], "depth")
    fails(blocks, [dict(good, partner=[0, 0])], "permutation")
    fails(blocks, [dict(good, partner=[0, 2])], "permutation")
    for field, entry, needle in (("subs", (8, "A"), "substitution beyond"), ("dels", (7, 2), "deletion beyond"), ("inss", (9, "A"), "insertion beyond")):
        broken = copy.deepcopy(blocks)
        broken[0]["members"][1][field].append(entry)
        fails(broken, [good], needle)
    # NULL lists with a count, and a merged consensus of 2^30 letters: the raw call (lengths are read before any letter is)
    K = _Packed(blocks, [])
    args = list(K.args()[:7])
    dll = gpu_lib.dll
    for null_at in (2, 3, 4, 5, 6):
        a = list(args)
        a[null_at] = None
        with pytest.raises(batch.PgaError):
            sp.merge_blocks_raw(a, [(0, 1, 0, 1)], [1, 0], dll)
    K.B[0].cons_len = (1 << 30) - 3
    with pytest.raises(batch.PgaError):
        sp.merge_blocks_raw(args, [(0, 1, 0, 1)], [1, 0], dll)
    K.B[0].cons_len = 8
    out = sp.merge_blocks_raw(args, [], [], dll)                                          # no edge: empty lists, no device call
    assert out.to_dicts() == []
    out.free()
    check_batch(dll, blocks, [good])


# ---------------------------------------------------------------- 4. the plasmid graph, round by round
@pytest.fixture(scope="module")
def plasmids():
    G = json.load(gzip.open(os.path.join(GOLDEN, "plasmids.json.gz")))
    names = [G["paths"][k]["name"] for k in sorted(G["paths"], key=int)]
    return G, names, dict(zip(*rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))))


@pytest.mark.parametrize("n_paths", [1, 3, 8])
def test_plasmids_device_rounds(gpu_lib, plasmids, n_paths):
    G, names, genome = plasmids
    focal = names[:n_paths]
    trace = {}
    g = sp.simplify(G, focal, dll=gpu_lib.dll, trace=trace)
    assert g == sr.simplify(sr.from_json(G), set(focal), trace["rounds"])       # blocks, edits in list order, nodes and paths
    assert not sp.find_transitive_edges(g) and len(trace["zero_copy"]) == len(trace["rounds"])
    blocks, paths, kept = sg.recon_input(g)
    res = reconstruct(blocks, paths, [genome[n] for n in kept], want_seqs=False, dll=gpu_lib.dll)
    assert [(r["status"], r["n_mismatch"]) for r in res] == [(0, 0)] * n_paths


def test_a_round_reads_the_previous_output_in_place(gpu_lib, plasmids):
    """the first path alone: the second round is restricted to edges between blocks the first round built, so that its input is the first
    round's output arrays as they are; and pga_reconstruct reads a round's output the same way"""
    G, names, genome = plasmids
    focal = names[:1]
    first = {}
    sp.simplify(G, focal, merge=sr.merge_batch, trace=first)
    r1 = first["rounds"][0]
    g = sr.from_json(G)
    for pid in [pid for pid, p in g["paths"].items() if p["name"] not in focal]:
        sr.remove_path(g, pid)
    built = set()
    for e in r1:
        built.add(sr.orient_merging_edge(g, e)[0][0])
        sr.merge_blocks(g, e)
    r2 = sp.choose_round([e for e in sp.find_transitive_edges(g) if e[0][0] in built and e[1][0] in built])
    assert len(r2) >= 2
    trace = {}
    got = sp.simplify(G, focal, dll=gpu_lib.dll, schedule=[r1, r2], trace=trace)
    assert trace["rounds"][:2] == [r1, r2] and trace["zero_copy"][:2] == [False, True]
    assert got == sr.simplify(sr.from_json(G), set(focal), trace["rounds"])
    # pga_reconstruct over a call's output by pointer: every output member as a path of one node
    blocks, edges = sg.edge_batch()
    exp = sr.merge_batch(blocks, edges)
    K = _Packed(blocks, [])
    out = sp.merge_blocks_raw(K.args()[:7], [(e["left"], e["right"], e["left_rc"], e["right_rc"]) for e in edges], [q for e in edges for q in e["partner"]], gpu_lib.dll, keep=K)
    try:
        n = sum(out.n_members)
        want = [rr._apply_keeping_gaps(r["consensus"], m) for r in exp for m in r["members"]]

        class View:
            n_paths = n
            P = (recon_path_t * max(n, 1))(*[recon_path_t(len(s), 0, 1, 0) for s in want])
            N = (recon_node_t * max(n, 1))(*[recon_node_t(k, 0, 0) for k in range(n)])

            def args(self):
                return out.graph_args() + (n, self.P, self.N)

        res = reconstruct_packed(View(), want, want_seqs=True, dll=gpu_lib.dll)
        assert [(r["status"], r["n_mismatch"], r["seq"]) for r in res] == [(0, 0, s) for s in want]
    finally:
        out.free()
