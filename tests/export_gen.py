"""Graphs for the tests of the two export entries (tests/test_gpu_export.py), in the shape tests/export_ref.py takes: blocks, member_path,
n_paths, guide_path, guide_nodes.  Deterministic: a seed gives a graph."""
import random

IUPAC = "ACGTYRWSKMDVHBN"
UNIT_EDGE_LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097)


def E(inss=(), dels=(), subs=()):
    return {"inss": list(inss), "dels": list(dels), "subs": list(subs)}


def _letters(rng, n, odd=0.0):
    """mostly ACGT, some IUPAC; with probability `odd` per letter a lower-case letter or an X (the complement rejects them)"""
    return "".join(rng.choice("xXa") if odd and rng.random() < odd else rng.choice(IUPAC) if rng.random() < 0.1 else rng.choice("ACGT") for _ in range(n))


def _edits(rng, L, odd, gap_subs):
    """overlapping and adjacent deletions, substitutions under deletions and at both ends, repeated positions, insertions (two at one
    position too); gap_subs: the probability of a literal '-' substitution"""
    e = E()
    if L:
        shape = rng.randrange(8)
        for _ in range(rng.randrange(4) if shape < 6 else 0):
            pos = rng.randrange(L)
            ln = rng.randrange(min(L - pos, 30) + 1)
            e["dels"].append((pos, ln))
            if shape == 1 and pos + ln < L:
                e["dels"].append((pos + ln, rng.randrange(min(L - pos - ln, 20) + 1)))      # adjacent
            if shape == 2 and ln:
                e["dels"].append((pos + rng.randrange(ln), rng.randrange(1, min(L - pos - ln, 10) + 2) if pos + ln < L else 1))   # overlapping
            if ln and rng.random() < 0.5:
                e["subs"].append((pos + rng.randrange(ln), "G"))                            # under the deletion
        if shape == 3 and L <= 70:
            e["dels"].append((0, L))                                                        # the whole consensus
        for _ in range(rng.randrange(5)):
            pos = rng.choice((0, L - 1)) if rng.random() < 0.3 else rng.randrange(L)
            e["subs"].append((pos, _letters(rng, 1, odd)))
            if rng.random() < 0.3:
                e["subs"].append((pos, _letters(rng, 1)))
        if rng.random() < gap_subs:
            e["subs"].append((rng.randrange(L), "-"))
        rng.shuffle(e["subs"])
    for _ in range(rng.randrange(3)):
        pos = rng.randrange(L + 1)
        e["inss"].append((pos, _letters(rng, rng.choice((0, 1, 3, 17, 40)), odd)))
        if rng.random() < 0.25:
            e["inss"].append((pos, _letters(rng, rng.randrange(1, 20))))
    return e


def random_graph(seed):
    """1-6 paths, 1-8 blocks, consensus lengths 0-70 and a few between 4000 and 4200, blocks visited twice or missing from a path (not
    core), about half of the guide's nodes reverse, IUPAC letters, a few lower-case / X letters and a few literal '-' substitutions;
    -> dict(blocks, member_path, n_paths, guide_path, guide_nodes), order_rows (a permutation of the paths), order_members"""
    rng = random.Random(1000 + seed)
    n_paths, n_blocks = rng.randrange(1, 7), rng.randrange(1, 9)
    odd = 0.004 if seed % 4 == 0 else 0.0
    gap_subs = 0.08 if seed % 3 == 0 else 0.0
    blocks, member_path = [], []
    for b in range(n_blocks):
        L = rng.randrange(4000, 4201) if rng.random() < 0.12 else rng.randrange(0, 71)
        kind = rng.random()
        if kind < 0.7 or b == 0 and seed % 5:
            on = list(range(n_paths))                                                       # once in every path: core
        elif kind < 0.85:
            on = [p for p in range(n_paths) if rng.random() < 0.6]                          # missing from some paths
        else:
            on = list(range(n_paths)) + [rng.randrange(n_paths)]                            # visited twice by one path
        rng.shuffle(on)
        if not on:
            on = [rng.randrange(n_paths)]
        blocks.append({"consensus": _letters(rng, L, odd), "members": [_edits(rng, L, odd, gap_subs) for _ in on]})
        member_path += on
    guide_path = rng.randrange(n_paths)
    guide_nodes, m = [], 0
    for b, blk in enumerate(blocks):
        for j in range(len(blk["members"])):
            if member_path[m] == guide_path:
                guide_nodes.append((b, j, rng.random() < 0.5))
            m += 1
    rng.shuffle(guide_nodes)
    order_rows = list(range(n_paths)); rng.shuffle(order_rows)
    order_members = list(range(len(member_path))); rng.shuffle(order_members)
    return dict(blocks=blocks, member_path=member_path, n_paths=n_paths, guide_path=guide_path, guide_nodes=guide_nodes), order_rows, order_members


def edge_graph():
    """three paths over core blocks whose consensus lengths are UNIT_EDGE_LENGTHS (a row of each length as a block-sequence row; rows over
    several of them as core rows, with a zero-length piece between two others) and over blocks of 100 letters with one deletion each that starts or
    ends at offsets 15, 16, 17 of a unit or covers whole units; a deletion of a whole consensus; substitutions at the first and at the last
    letter, twice at one position and under a deletion.  The guide reads every other block in reverse."""
    rng = random.Random(7)
    blocks = []
    for L in UNIT_EDGE_LENGTHS:
        ends = E(subs=[(0, "T"), (L - 1, "G"), (L - 1, "C")]) if L else E()
        gone = E(dels=[(0, L)], subs=[(L // 2, "T")]) if L else E()
        blocks.append({"consensus": _letters(rng, L), "members": [E(), ends, gone]})
    for s in (0, 15, 16, 17, 31, 32, 33):
        for e in (15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 100):
            if e > s:
                behind = [(e, "T"), (e, "R")] if e < 100 else []
                blocks.append({"consensus": _letters(rng, 100), "members": [E(dels=[(s, e - s)], subs=[(s, "G")] + behind), E(), E(dels=[(s, e - s), (max(s - 3, 0), 5)])]})
    member_path = [p for _ in blocks for p in (0, 1, 2)]
    guide_nodes = [(b, 1, b % 2 == 1) for b in range(len(blocks))]        # path 1; block 0 (no letters) lies between pieces of other rows' ends
    guide_nodes = guide_nodes[1:3] + guide_nodes[:1] + guide_nodes[3:]   # the empty block between two others
    return dict(blocks=blocks, member_path=member_path, n_paths=3, guide_path=1, guide_nodes=guide_nodes)


def big_graph(n_paths=6, n_blocks=50, mean=1000, seed=11):
    """about n_paths * n_blocks * mean letters, every block core, a third of the guide's nodes reverse"""
    rng = random.Random(seed)
    blocks, member_path = [], []
    for b in range(n_blocks):
        L = rng.randrange(mean * 8 // 10, mean * 12 // 10)
        on = list(range(n_paths)); rng.shuffle(on)
        blocks.append({"consensus": _letters(rng, L), "members": [_edits(rng, L, 0.0, 0.0) for _ in on]})
        member_path += on
    guide_nodes = [(b, member_path[b * n_paths:(b + 1) * n_paths].index(2), rng.random() < 0.33) for b in range(n_blocks)]
    rng.shuffle(guide_nodes)
    return dict(blocks=blocks, member_path=member_path, n_paths=n_paths, guide_path=2, guide_nodes=guide_nodes)


def check_segments(collector, res_len):
    """the segments a sink saw tile every non-empty row exactly once, in order, inside their tiles and without overlap there; -> the rows in
    the order they were delivered"""
    at = [0] * len(res_len)
    delivered = []
    for s, t in zip(collector.segs, collector.letters):
        used = 0
        for row, row_off, tile_off, n, _ in s.tolist():
            assert n > 0 and row_off == at[row] and tile_off >= used and tile_off % 16 == 0 and tile_off + n <= len(t), (row, row_off, tile_off, n)
            if row_off == 0:
                delivered.append(row)
            else:
                assert delivered[-1] == row                                                   # a row goes on where the last tile left it
            at[row] += n
            used = tile_off + n
    assert at == list(res_len)
    assert len(delivered) == len(set(delivered)) == sum(1 for n in res_len if n)
    return delivered
