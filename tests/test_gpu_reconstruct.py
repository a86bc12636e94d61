"""pga_reconstruct (reconstruct_run.rs:56-127 on the device: k_reconstruct, pga_reconstruct.hip) against the restatement
tests/reconstruct_ref.py and against a graph the reference wrote (tests/golden/plasmids.json.gz spells tests/golden/plasmids.fa.gz).
Every comparison is exact."""
import os

import numpy as np
import pytest

import mapvarbind as mb
import promise_ref as pr
import reconstruct_ref as rr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

from pangraph_amd.reconstruct import LETTERS, TILE  # noqa: E402

assert (TILE, LETTERS) == (4096, 16)


def E(inss=(), dels=(), subs=()):
    return {"inss": list(inss), "dels": list(dels), "subs": list(subs)}


def P(nodes, tot_len, first_pos=0):
    return {"nodes": list(nodes), "tot_len": tot_len, "first_pos": first_pos}


def member_len(blocks, b, m):
    return len(rr._apply_keeping_gaps(blocks[b]["consensus"], blocks[b]["members"][m]))


def path_of(blocks, nodes, first_pos=0):
    """a consistent path over `nodes`: tot_len is what they add up to"""
    return P(nodes, sum(member_len(blocks, b, m) for b, m, _ in nodes), first_pos)


def plant(seq, positions):
    s = list(seq)
    for i in positions:
        s[i] = "A" if s[i] != "A" else "C"
    return "".join(s)


def check(dll, blocks, paths, expected=None, want_seqs=True):
    from pangraph_amd.reconstruct import reconstruct
    got = reconstruct(blocks, paths, expected, want_seqs, dll=dll)
    exp = rr.expected_results(blocks, paths, expected, want_seqs)
    assert len(got) == len(exp) == len(paths)
    for i, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (i, paths[i]["tot_len"], paths[i]["first_pos"], len(paths[i]["nodes"]), {k: (g[k], e[k]) for k in g if k != "seq" and g[k] != e[k]})
    return got


# ---------------------------------------------------------------- 1. the plasmid graph
@pytest.fixture(scope="module")
def plasmids():
    from pangraph_amd.reconstruct import graph_from_json
    blocks, paths, names = graph_from_json(os.path.join(GOLDEN, "plasmids.json.gz"))
    by_name = dict(zip(*rr.read_fasta(os.path.join(GOLDEN, "plasmids.fa.gz"))))
    return blocks, paths, [by_name[n] for n in names]


def test_plasmid_graph_write_and_verify(gpu_lib, plasmids):
    from pangraph_amd.reconstruct import reconstruct
    blocks, paths, fasta = plasmids
    assert len(paths) == 15
    got = reconstruct(blocks, paths, dll=gpu_lib.dll)                                  # write mode
    assert [g["status"] for g in got] == [0] * 15
    assert [g["seq"] for g in got] == fasta
    got = reconstruct(blocks, paths, expected=fasta, want_seqs=False, dll=gpu_lib.dll)  # verify mode, nothing downloaded
    assert [(g["status"], g["len"], g["seq"], g["first_mismatch"], g["n_mismatch"]) for g in got] == [(0, len(s), None, -1, 0) for s in fasta]


def test_plasmid_graph_planted_differences(gpu_lib, plasmids):
    from pangraph_amd.reconstruct import reconstruct
    blocks, paths, fasta = plasmids
    planted, where = [], []
    for i, (p, s) in enumerate(zip(paths, fasta)):
        assert len(s) > TILE + 1 and 0 < p["first_pos"] < len(s)
        every = [0, len(s) - 1, p["first_pos"] - 1, p["first_pos"], TILE - 1, TILE]
        pos = sorted(set(every if i % 5 == 0 else [every[(i + k) % 6] for k in range(i % 4)]))   # all six, some of them, none (i = 4, 8, 12)
        where.append(pos); planted.append(plant(s, pos))
    assert any(not w for w in where) and any(len(w) == 6 for w in where)
    got = reconstruct(blocks, paths, expected=planted, dll=gpu_lib.dll)                 # both modes in one call
    for g, s, bad, w in zip(got, fasta, planted, where):
        assert (g["first_mismatch"], g["n_mismatch"]) == rr.compare(s, bad) == (w[0] if w else -1, len(w))
        assert g["status"] == 0 and g["seq"] == s


# ---------------------------------------------------------------- 2. edge shapes, one call
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, TILE - 1, TILE, TILE + 1)


def edge_graph():
    rng = np.random.default_rng(11)
    L = TILE + 80
    cons = mb.random_seq(rng, L)
    ALL = LENGTHS + (TILE - 32,)
    A = {"consensus": cons, "members": [E(dels=[(n, L - n)]) for n in ALL] + [E(dels=[(0, L - n)]) for n in ALL]}     # the first n letters, the last n
    nA = len(ALL)
    at = {n: i for i, n in enumerate(ALL)}
    small = {"consensus": "ACGTTGCA", "members": [E(dels=[(1, 7)]), E(dels=[(0, 6)]), E(dels=[(2, 5)]), E(dels=[(0, 8)]), E(dels=[(0, 5), (3, 5)], subs=[(4, "T")])]}   # 1, 2, 3, 0, 0 letters
    c100 = mb.random_seq(rng, 100)
    big = mb.random_seq(rng, 5000)
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    shapes = {"consensus": c100, "members": [                                           # the member edit shapes of test_gpu_promise.py::test_stage_jobs_on_edge_shapes
        E(inss=[(0, "ACGGT")]), E(inss=[(100, "TTGCA")]), E(inss=[(0, "AC"), (100, "GT")]),
        E(inss=[(5, "TT"), (5, "AC")]), E(inss=[(5, "AC"), (5, "A"), (5, "ACG")]),
        E(inss=[(50, big)]), E(inss=[(0, big)], dels=[(0, 100)]),
        E(dels=[(0, 3)]), E(dels=[(97, 3)]), E(dels=[(0, 3), (97, 3)]),
        E(dels=[(10, 5), (15, 5)]), E(dels=[(15, 5), (10, 5)]), E(dels=[(10, 10), (15, 10)]), E(dels=[(10, 0), (10, 4)]),
        E(dels=[(10, 5)], subs=[(12, other[c100[12]])]),
        E(subs=[(7, other[c100[7]]), (7, other[other[c100[7]]])]),
        E(subs=[(99, other[c100[99]]), (0, other[c100[0]]), (50, other[c100[50]])]),
        E(dels=[(10, 10)], inss=[(15, "ACG")]), E(dels=[(10, 10)], inss=[(10, "AC"), (20, "GT")]),
        E(inss=[(30, "YKM"), (60, "RWSN")], subs=[(1, "R"), (2, "B")]),
        E(dels=[(0, 100)]), E(dels=[(0, 100)], inss=[(40, "ACGT")]), E(),
    ]}
    iupac = "ACGTYRWSKMDVHBN" * 5
    I = {"consensus": iupac, "members": [E(), E(dels=[(3, 7)], inss=[(20, "HDVB")], subs=[(0, "N")])]}
    blocks = [A, small, shapes, I]
    paths = []
    # every length with every rotation that is valid for it, forward and reverse, from both ends of the consensus
    for j, n in enumerate(LENGTHS):
        for fp in sorted(set(x for x in (0, 1, 15, 16, 17, n - 1, n) if 0 <= x <= n)):
            paths.append(P([(0, at[n] + (nA if (j + fp) % 2 else 0), (j + fp) % 3 == 0)], n, fp))
    # node boundaries on 16-letter and tile boundaries, rotations on and off them
    chain = [(0, at[16], False), (0, at[16], True), (0, at[TILE - 32], False), (0, at[TILE], True), (0, at[64] + nA, False), (0, at[TILE - 1], True), (0, at[1], False), (0, at[17], True)]
    tot = 3 * TILE + 81                                                                 # node boundaries at 16, 32, TILE, 2 TILE, 2 TILE + 64, 3 TILE + 63, 3 TILE + 64
    assert tot == sum(n for n in (16, 16, TILE - 32, TILE, 64, TILE - 1, 1, 17))
    for fp in (0, 16, 32, TILE, 2 * TILE, 2 * TILE + 64, tot - 1, tot, 7):
        paths.append(P(chain, tot, fp))
    # 300 nodes of 1-3 letters, strands mixed: one thread spans several nodes
    tiny = [(1, int(rng.integers(0, 3)), bool(rng.integers(0, 2))) for _ in range(300)]
    for fp in (0, 5, 16, 299):
        paths.append(path_of(blocks, tiny, fp))
    # empty nodes first, in the middle and last; no nodes; only empty nodes; one member named by two nodes
    paths.append(path_of(blocks, [(1, 3, False), (1, 0, False), (1, 4, True), (1, 3, True), (1, 2, True), (1, 4, False)], 2))
    paths.append(P([], 0, 0)); paths.append(P([], 123, 45))
    paths.append(P([(1, 3, False), (1, 4, True), (2, 20, False)], 0, 0))
    paths.append(path_of(blocks, [(2, 5, False), (2, 5, True), (2, 5, False), (0, at[65], True), (0, at[65], True)], 5003))
    # the edit shapes, every one alone (both strands) and all in a chain
    for m in range(len(shapes["members"])):
        for rev in (False, True):
            p = path_of(blocks, [(2, m, rev)])
            p["first_pos"] = p["tot_len"] // 3
            paths.append(p)
    paths.append(path_of(blocks, [(2, m, m % 3 == 1) for m in range(len(shapes["members"]))] + [(3, 0, True), (3, 1, False), (3, 1, True)], 4097))
    return blocks, paths


def test_edge_shapes_in_one_call(gpu_lib):
    blocks, paths = edge_graph()
    assert len(paths) > 120
    plain = rr.expected_results(blocks, paths)
    assert all(r["status"] == 0 for r in plain) and {0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1} <= set(r["len"] for r in plain)
    check(gpu_lib.dll, blocks, paths)                                                   # write mode
    exact = [r["seq"] for r in plain]
    check(gpu_lib.dll, blocks, paths, exact, want_seqs=False)                            # verify mode
    # both modes, every third path with differences planted: first and last letter, both sides of the seam, both sides of a 16-letter edge
    bad = []
    for i, (p, s) in enumerate(zip(paths, exact)):
        pos = sorted(set(x for x in (0, len(s) - 1, p["first_pos"] - 1, p["first_pos"], 15, 16) if 0 <= x < len(s))) if i % 3 == 0 else []
        bad.append(plant(s, pos))
    got = check(gpu_lib.dll, blocks, paths, bad)
    assert sum(g["n_mismatch"] for g in got) > 100 and [g["seq"] for g in got] == exact


# ---------------------------------------------------------------- 3. statuses
def test_statuses(gpu_lib):
    rng = np.random.default_rng(3)
    c = mb.random_seq(rng, 200)
    good = {"consensus": c, "members": [E(), E(dels=[(10, 30)], inss=[(100, "ACGTT")]), E(subs=[(199, "-")], dels=[(190, 10)]), E(subs=[(5, "X")], dels=[(5, 1)])]}
    alien = {"consensus": c[:50] + "X" + c[51:], "members": [E(), E(dels=[(50, 1)])]}              # X in the consensus
    lower = {"consensus": c, "members": [E(subs=[(7, "a")]), E(inss=[(9, "AXA")])]}
    gaps = {"consensus": c[:20] + "-" + c[21:], "members": [E(), E(dels=[(20, 1)])]}                # '-' in the consensus, and hidden by a deletion
    gaps2 = {"consensus": c, "members": [E(inss=[(30, "A-A")]), E(subs=[(40, "-")])]}
    blocks = [good, alien, lower, gaps, gaps2]
    ok0, ok1 = path_of(blocks, [(0, 0, False), (0, 1, True)], 77), path_of(blocks, [(0, 1, False), (0, 2, True), (0, 3, True)], 3)
    paths = [
        ok0,
        P([(0, 0, False)], 199),                                                        # 1
        P([(1, 0, True)], 200), P([(2, 0, True)], 200), P([(2, 1, True)], 203),         # 2: X in the consensus, lower case, X in an insertion
        P([(3, 0, False)], 200), P([(3, 0, True)], 200), P([(4, 0, False)], 203), P([(4, 1, True)], 200),   # 3
        P([(0, 0, False)], 200, 201),                                                   # 4
        P([(1, 0, True)], 1), P([(1, 0, True), (3, 0, False)], 400), P([(3, 0, False)], 7), P([(0, 0, False)], 199, 500),   # 2 with 1, 2 with 3, 3 with 1, 1 with 4
        P([(1, 0, False)], 200, 9), P([(2, 0, False), (2, 1, False)], 403, 1),          # forward: X and lower case pass through
        P([(1, 1, True)], 199), P([(3, 1, True)], 199, 199),                            # the X and the '-' under a deletion: 0
        ok1,
    ]
    exp_status = [0, 1, 2, 2, 2, 3, 3, 3, 3, 4, 2, 2, 3, 1, 0, 0, 0, 0, 0]
    plain = rr.expected_results(blocks, paths)
    assert [r["status"] for r in plain] == exp_status
    got = check(gpu_lib.dll, blocks, paths)
    assert [g["status"] for g in got] == exp_status and got[14]["seq"][9 + 50] == "X" and "a" in got[15]["seq"]
    # verify mode: 5 alone, 5 behind every other status, and the good paths compared
    expected = [r["seq"] if r["status"] == 0 else "ACGT" for r in plain]
    expected[0] = expected[0][:-1]; expected[16] = expected[16] + "A"
    got = check(gpu_lib.dll, blocks, paths, expected, want_seqs=False)
    assert [g["status"] for g in got] == [5] + exp_status[1:16] + [5] + exp_status[17:]
    assert all((g["first_mismatch"], g["n_mismatch"]) == (-1, 0) for g in got)


# ---------------------------------------------------------------- 4. random graphs
def random_edit(rng, cons):
    L = len(cons)
    subs = [(int(p), "ACGT"[int(rng.integers(0, 4))]) for p in rng.integers(0, L, max(1, L // 100))]
    dels = [(int(p), int(min(rng.integers(0, 25), L - p))) for p in rng.integers(0, L, int(rng.integers(0, 4)))]
    inss = [(int(p), mb.random_seq(rng, int(rng.integers(1, 40)))) for p in rng.integers(0, L + 1, int(rng.integers(0, 4)))]
    return E(inss, dels, subs)


def random_graph(seed, n_blocks, n_paths, letters):
    rng = np.random.default_rng(seed)
    blocks = []
    for _ in range(n_blocks):
        cons = mb.random_seq(rng, int(rng.integers(100, 3000)))
        blocks.append({"consensus": cons, "members": [random_edit(rng, cons) for _ in range(int(rng.integers(2, 16)))]})
    built = {}

    def seq_of(b, m, rev):
        if (b, m) not in built:
            built[(b, m)] = rr._apply_keeping_gaps(blocks[b]["consensus"], blocks[b]["members"][m])
        return pr.reverse_complement(built[(b, m)]) if rev else built[(b, m)]
    paths, seqs = [], []
    for _ in range(n_paths):
        nodes, parts, n = [], [], 0
        while n < letters // n_paths:
            b = int(rng.integers(0, n_blocks)); node = (b, int(rng.integers(0, len(blocks[b]["members"]))), bool(rng.random() < 0.3))
            nodes.append(node); parts.append(seq_of(*node)); n += len(parts[-1])
        genome = "".join(parts)
        fp = int(rng.integers(0, len(genome) + 1))
        paths.append(P(nodes, len(genome), fp)); seqs.append(rr.rotate_right(genome, fp))
    return blocks, paths, seqs


def test_random_graph_vs_restatement(gpu_lib):
    blocks, paths, seqs = random_graph(101, 30, 20, 200_000)
    assert sum(len(b["members"]) for b in blocks) > 150 and 180_000 < sum(len(s) for s in seqs) < 300_000
    got = check(gpu_lib.dll, blocks, paths)                                             # the restatement, node by node
    assert [g["seq"] for g in got] == seqs
    bad = [plant(s, [0, len(s) // 2, len(s) - 1][: i % 4]) for i, s in enumerate(seqs)]
    check(gpu_lib.dll, blocks, paths, bad, want_seqs=False)


def test_chunked_run_equals_one_chunk(gpu_lib):
    from pangraph_amd.reconstruct import reconstruct
    blocks, paths, seqs = random_graph(202, 40, 20, 3_000_000)
    assert sum(len(s) for s in seqs) > 2_900_000 and max(len(s) for s in seqs) < (1 << 20)       # every chunk of 1 MB holds several paths, none holds all
    bad = [plant(s, [len(s) // 3, len(s) - 1][: i % 3]) for i, s in enumerate(seqs)]
    whole = reconstruct(blocks, paths, expected=bad, dll=gpu_lib.dll)
    assert [g["seq"] for g in whole] == seqs
    assert [(g["first_mismatch"], g["n_mismatch"]) for g in whole] == [rr.compare(s, b) for s, b in zip(seqs, bad)]
    old = os.environ.get("PGA_RECON_CHUNK_MB")
    os.environ["PGA_RECON_CHUNK_MB"] = "1"                                               # (the library reads it at every call)
    try:
        chunked = reconstruct(blocks, paths, expected=bad, dll=gpu_lib.dll)
        chunked_verify = reconstruct(blocks, paths, expected=bad, want_seqs=False, dll=gpu_lib.dll)
    finally:
        if old is None:
            del os.environ["PGA_RECON_CHUNK_MB"]
        else:
            os.environ["PGA_RECON_CHUNK_MB"] = old
    assert chunked == whole
    assert chunked_verify == [dict(g, seq=None) for g in whole]


# ---------------------------------------------------------------- 5. malformed inputs
def test_malformed_inputs_fail_the_call(gpu_lib):
    """every case is rejected by the validation at the top of reconstruct_host (pga_reconstruct.hip), before anything is launched"""
    import ctypes as C
    from pangraph_amd.batch import PgaError
    from pangraph_amd.reconstruct import _Packed, reconstruct, reconstruct_packed
    dll = gpu_lib.dll
    c = "ACGTACGTAC"
    blocks = [{"consensus": c, "members": [E(), E(subs=[(3, "T")], dels=[(5, 2)], inss=[(10, "GG")])]}]
    paths = [P([(0, 0, False), (0, 1, True)], 20, 4)]
    good = rr.expected_results(blocks, paths)

    def bad_edit(e, what):
        with pytest.raises(PgaError, match=what):
            reconstruct([{"consensus": c, "members": [E(), e]}], paths, dll=dll)
        assert reconstruct(blocks, paths, dll=dll) == good                               # the library is still usable
    bad_edit(E(subs=[(10, "A")]), "substitution beyond the consensus")
    bad_edit(E(dels=[(8, 3)]), "deletion beyond the consensus")
    bad_edit(E(inss=[(11, "A")]), "insertion beyond the consensus")
    with pytest.raises(PgaError, match="member that does not exist"):
        reconstruct(blocks, [P([(0, 0, False), (0, 2, False)], 20)], dll=dll)
    with pytest.raises(PgaError, match="neither write mode"):
        reconstruct(blocks, paths, want_seqs=False, dll=dll)
    with pytest.raises(PgaError, match="null expected sequence with a non-zero length"):
        reconstruct_packed(_Packed(blocks, paths), [None], True, dll, expected_len=[20])
    K = _Packed(blocks, paths)
    K.B[0].consensus = None
    with pytest.raises(PgaError, match="null consensus with a non-zero length"):
        reconstruct_packed(K, dll=dll)
    for name, what in (("M", "null member list"), ("S", "null edit list"), ("D", "null edit list"), ("I", "null edit list"), ("L", "null insertion letters"),
                       ("P", "null path list"), ("N", "null node list")):
        K = _Packed(blocks, paths)
        setattr(K, name, None)
        with pytest.raises(PgaError, match=what):
            reconstruct_packed(K, dll=dll)
    # a path longer than 2^31 letters: 2^21 + 1 nodes of one member of 1024 letters (the lengths are added up on the host; nothing is built)
    kb = mb.random_seq(np.random.default_rng(5), 1024)
    K = _Packed([{"consensus": kb, "members": [E()]}], [P([], 0)])
    n = (1 << 21) + 1
    K.N = (type(K.N[0]) * n)()                                                           # (zeroed: member 0, forward)
    K.P[0].n_nodes = n; K.P[0].tot_len = n * 1024
    with pytest.raises(PgaError, match="path longer than 2\\^31 letters"):
        reconstruct_packed(K, dll=dll)
    assert reconstruct(blocks, paths, expected=[good[0]["seq"]], dll=dll) == [dict(good[0], first_mismatch=-1, n_mismatch=0)]
    assert C.sizeof(K.N) == 16 * n
