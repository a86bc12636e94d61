"""Levels for the tests of pga_plan_merge: (groups, matches) as pangraph_amd.reweave.plan_merge and reweave_ref.expected_call take them.
A block is laid out as a list of pieces, ("g", n) a gap of n letters, ("h", n, key) a hit of n letters; every key appears exactly twice in
its group, on two different blocks: the first occurrence (in block order) is the ref hit unless pairs[key]["qry_first"].  The layout makes
hits that do not overlap by construction."""
import random

THR = 20
CIGAR_LENGTHS = (1, 2, 63, 64, 65, 3001)
HIT_COUNTS = (1, 2, 63, 64, 65)


def letters(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def random_cigar(rng, n, kinds="MID=X"):
    return [(rng.choice(kinds), rng.randint(1, 30)) for _ in range(n)]


class Level:
    def __init__(self, seed):
        self.rng, self.groups, self.matches = random.Random(seed), [], []

    def group(self, layouts, pairs=None, ids=None, depths=None, consensus=None):
        """layouts: per block its pieces; pairs: {key: {"reverse", "cigar", "qry_first"}} (missing entries are drawn); -> the group's index"""
        rng, g = self.rng, len(self.groups)
        pairs = dict(pairs or {})
        blocks, seen = [], {}
        for b, pieces in enumerate(layouts):
            at = 0
            for p in pieces:
                if p[0] == "h":
                    seen.setdefault(p[2], []).append((b, at, at + p[1]))
                at += p[1]
            blocks.append({"block_id": ids[b] if ids else rng.randrange(1 << 63), "depth": depths[b] if depths else 1,
                           "consensus": consensus[b] if consensus and consensus[b] is not None else letters(rng, at)})
            assert len(blocks[-1]["consensus"]) == at
        for key, occ in seen.items():
            assert len(occ) == 2 and occ[0][0] != occ[1][0], key
            q = pairs.get(key, {})
            ref, qry = (occ[1], occ[0]) if q.get("qry_first") else (occ[0], occ[1])
            cigar = q["cigar"] if "cigar" in q else random_cigar(rng, rng.choice((1, 3, 8)))
            self.matches.append({"group": g, "qry": qry[0], "ref": ref[0], "qry_start": qry[1], "qry_end": qry[2], "ref_start": ref[1], "ref_end": ref[2],
                                 "reverse": bool(q["reverse"]) if "reverse" in q else bool(rng.randrange(2)), "cigar": cigar})
        self.groups.append(blocks)
        return g

    def level(self):
        return self.groups, self.matches


def _many_hits(counts, thr=THR):
    """one block with counts[k] hits each, every hit paired with its own small block; gaps between the hits from the edges of the rule"""
    gaps = (0, thr, thr + 3, 0, 2 * thr)
    layouts, key = [], 0
    partners = []
    for n in counts:
        pieces = []
        for t in range(n):
            pieces += [("g", gaps[(t + n) % len(gaps)]), ("h", thr + (t * 7) % 11, key)]
            partners.append([("h", thr + (t * 5) % 13, key)])
            key += 1
        layouts.append(pieces)
    return layouts + partners


def hits_level():
    """blocks with 1, 2, 63, 64, 65 hits (the scans cross a wave and a workgroup: 195 hits on 5 blocks, 390 hits in all); two groups that
    reuse the same block ids; a group without matches; a block without a hit"""
    L = Level(11)
    layouts = _many_hits(HIT_COUNTS)
    ids = [1000000 - 7 * k for k in range(len(layouts))]                       # (descending: the output order is not the input order)
    L.group(layouts, ids=ids)
    L.group([[("g", 50)], [("g", 7)]], ids=[5, 4])                           # no matches
    L.group(layouts + [[("g", 33)]], ids=ids + [3])                          # the same ids again, and a block without a hit
    return L.level()


def promise_levels():
    """63 / 64 / 65 promises in one group"""
    out = []
    for n in (63, 64, 65):
        L = Level(100 + n)
        L.group([[("h", THR + k % 5, k) for k in range(n)], [("h", THR + k % 3, n - 1 - k) for k in range(n)]])
        out.append(L.level())
    return out


def refine_level(thr=THR):
    """every rule of refine_intervals on blocks that succeed: gaps of thr - 1 and thr, equal left and right lengths (left wins), a short
    gap at block start and at block end, adjacent hits, one hit receiving both extensions"""
    L = Level(21)
    s = thr - 1
    layouts = [
        [("g", s), ("h", thr + 5, 0), ("g", thr), ("h", thr + 5, 1), ("g", s), ("h", thr + 5, 2), ("g", s)],        # start, thr, equal lengths (left wins), end
        [("h", thr, 0), ("h", thr + 1, 1), ("h", thr + 2, 2)],                                                     # adjacent hits, no gap
        [("h", thr + 9, 3), ("g", 1), ("h", thr + 10, 4), ("g", s), ("h", thr + 9, 5)],                            # both gaps go to the longer middle hit
        [("g", 1), ("h", thr, 3), ("g", 1)], [("h", thr + 1, 4)], [("g", thr), ("h", thr + 2, 5), ("g", thr)],
        [("h", thr + 9, 6), ("g", 1), ("h", thr + 3, 7)],                                                          # the gap goes left (longer)
        [("h", thr, 6)], [("h", thr, 7)],
    ]
    L.group(layouts)
    return L.level()


def failing_blocks(thr=THR):
    """{name: layouts}: block 0 fails refine_intervals.  Codes 1 and 5 are the ones a block can report: a short gap whose LEFT neighbour is
    short (code 3) stands behind that neighbour in the list, and the neighbour, being aligned, has already failed with code 1."""
    s = thr - 1
    partners = lambda n: [[("h", thr, k)] for k in range(n)]
    return {
        "short_hit": [[("g", thr), ("h", s, 0), ("g", thr)]] + partners(1),                                   # 1 at index 1
        "short_hit_first": [[("h", s, 0)]] + partners(1),                                                     # 1 at index 0
        "gap_before_short_hit": [[("g", 2), ("h", s, 0)]] + partners(1),                                      # 5 at index 0: it precedes the hit's own code 1
        "gap_between": [[("h", thr, 0), ("g", 3), ("h", s, 1), ("g", thr), ("h", thr, 2)]] + partners(3),      # 5 at index 1
        "gap_behind_short_hit": [[("h", thr, 0), ("g", thr), ("h", s, 1), ("g", 3), ("h", thr, 2)]] + partners(3),   # 1 at index 2 (the gap behind would say 3)
        "short_hit_then_trailing": [[("h", thr, 0), ("g", thr), ("h", 1, 1), ("g", 2)]] + partners(2),         # 1 at index 2
        "later_block": [[("h", thr, 0)], [("g", thr), ("h", thr, 0), ("h", s, 1)], [("h", thr, 1)]],           # block 1 fails, block 0 does not
    }


def cigar_level(thr=THR):
    """one group per CIGAR case: two blocks, one match, all four flanks (each block [short gap][hit][short gap]) unless flanks is False;
    forward and reverse, ref and qry anchor"""
    rng = random.Random(31)
    cases = []
    for n in CIGAR_LENGTHS:
        cases.append(random_cigar(rng, n))
    cases += [
        [("I", 2), ("D", 3), ("I", 4), ("M", 10), ("D", 1), ("I", 2), ("D", 3)],      # the last of its kind before the first M is lengthened
        [("D", 2), ("I", 3), ("D", 4), ("M", 10), ("I", 1), ("D", 2), ("I", 3)],
        [("I", 5), ("D", 6)], [("D", 6)], [("I", 5)], [("D", 1), ("I", 2), ("D", 3), ("I", 4)],      # no M at all: the walk crosses the whole CIGAR
        [("M", 10)], [("=", 4), ("X", 1), ("=", 5)], [],
        [("I", 10), ("M", 100), ("D", 10), ("M", 10), ("D", 10)],                     # the base of test_update_cigar_forward / _reverse
    ]
    L = Level(32)
    for cg in cases:
        for reverse in (False, True):
            for deeper in (0, 1, 2):                                                  # ref deeper, qry deeper, equal
                for shape in (0, 1, 2):                                               # all four flanks; none; left flanks only
                    if shape and len(cg) > 70:
                        continue
                    a, z = (thr - 1, 3) if shape == 0 else (0, 0) if shape == 1 else (5, 0)
                    L.group([[("g", a), ("h", thr + 4, 0), ("g", z)], [("g", z and 2), ("h", thr + 6, 0), ("g", a and 1)]],
                            pairs={0: {"cigar": cg, "reverse": reverse}}, depths=[2 + (deeper == 0), 2 + (deeper == 1)])
    return L.level()


UPDATE_CIGAR_CASES = [
    # (base, anchor (left, right), append (left, right), reverse, expected): reweave.rs:1139-1204
    ("10M20D100M10I", (None, None), (None, None), False, "10M20D100M10I"),
    ("10I100M10D10M10D", (5, 10), (3, None), False, "5D13I100M10D10M20D"),
    ("10I100M10D10M10D", (5, 10), (3, None), True, "5D10I100M10D10M20D3I"),
]


def anchor_level():
    """the decision at equal depth: intervals inside one 16-bit word of the bit plane, straddling words, starting or ending on a multiple of
    16, length 1, the last base of the last sequence; R / Y without N; lower-case n; every group two blocks and one match"""
    L = Level(41)
    rng = L.rng

    def pair(c1, c2, i1, i2, depth=(2, 2)):
        """block 0 = c1 with the ref hit i1, block 1 = c2 with the qry hit i2"""
        lay = lambda n, iv: [("g", iv[0]), ("h", iv[1] - iv[0], 0), ("g", n - iv[1])]
        L.group([lay(len(c1), i1), lay(len(c2), i2)], consensus=[c1, c2], depths=list(depth), pairs={0: {"cigar": [("M", 5)]}})

    def with_n(n, at, letter="N"):
        s = list(letters(rng, n))
        for k in at:
            s[k] = letter
        return "".join(s)

    for iv in ((3, 9), (0, 16), (15, 17), (16, 32), (10, 40), (1, 2), (16, 17), (47, 48), (0, 100), (31, 100)):
        clean = letters(rng, 100)
        pair(clean, letters(rng, 100), iv, iv)                                            # nothing masked: the mask route
        pair(with_n(100, (iv[0],)), with_n(100, (iv[0], iv[1] - 1)), iv, iv)              # N on the first and last letter of the interval
        pair(with_n(100, (iv[0], iv[1] - 1)), with_n(100, (iv[1] - 1,)), iv, iv)          # qry has fewer
        pair(with_n(100, range(0, iv[0])) if iv[0] else clean, with_n(100, range(iv[1], 100)) if iv[1] < 100 else clean, iv, iv)   # N right outside: not counted
    pair(with_n(64, (5, 9), "R"), with_n(64, (7,), "Y"), (0, 64), (0, 64))                # masked, no N: letters route, counts 0, ref
    pair(with_n(64, (5,), "n"), letters(rng, 64), (0, 64), (0, 64))                       # lower case is not counted
    pair(with_n(64, (5,), "n"), with_n(64, (6,), "N"), (0, 64), (0, 64))
    pair(with_n(64, (5, 6), "N"), letters(rng, 64), (0, 64), (0, 64), depth=(3, 2))       # depth decides, the letters are not looked at
    pair(with_n(64, (5, 6), "N"), letters(rng, 64), (0, 64), (0, 64), depth=(2, 5))
    pair(letters(rng, 40), with_n(37, (36,)), (20, 40), (17, 37))                         # the last base of the last sequence of the batch
    return L.level()


ANCHOR_CASES = [
    # ((consensus 1, depth), (consensus 2, depth), (qry, qry interval, ref, ref interval), expected): reweave.rs:1212-1224
    (("ATCG", 2), ("NNCG", 2), (2, (0, 4), 1, (0, 4)), "ref"),
    (("ATCG", 2), ("NNCG", 2), (1, (0, 4), 2, (0, 4)), "qry"),
    (("ANCG", 2), ("TNCG", 2), (2, (0, 4), 1, (0, 4)), "ref"),
    (("ATCG", 2), ("GCTA", 2), (2, (0, 4), 1, (0, 4)), "ref"),
    (("NNNG", 2), ("NNCG", 2), (2, (0, 4), 1, (0, 4)), "qry"),
    (("NNCG", 3), ("ATCG", 2), (1, (0, 4), 2, (0, 4)), "qry"),
    (("NNCG", 3), ("ATCG", 2), (2, (0, 4), 1, (0, 4)), "ref"),
    (("ATCG", 10), ("ATCG", 2), (1, (0, 4), 2, (0, 4)), "qry"),
    (("NNNNNACGTNNNNN", 2), ("ACGTACNTACGT", 2), (2, (4, 8), 1, (5, 9)), "ref"),
    (("ACGN", 2), ("ACGT", 2), (1, (3, 4), 2, (3, 4)), "ref"),
    (("ACGT", 2), ("NCGT", 2), (2, (0, 1), 1, (0, 1)), "ref"),
]


def anchor_cases_level():
    """the eleven cases as one level, a group each (block ids 1 and 2)"""
    groups, matches = [], []
    for g, (b1, b2, (q, qi, r, ri), _) in enumerate(ANCHOR_CASES):
        groups.append([{"block_id": 1, "consensus": b1[0], "depth": b1[1]}, {"block_id": 2, "consensus": b2[0], "depth": b2[1]}])
        matches.append({"group": g, "qry": q - 1, "ref": r - 1, "qry_start": qi[0], "qry_end": qi[1], "ref_start": ri[0], "ref_end": ri[1], "reverse": False,
                        "cigar": [("M", 4)]})
    return groups, matches


def random_level(seed, thr=THR, fail=False):
    """up to 6 groups of up to 8 blocks; hits of thr .. thr + 40 letters, gaps from the edges of the rule (with fail: hits may be short)"""
    rng = random.Random(9000 + seed)
    L = Level(seed)
    for _ in range(rng.randint(1, 6)):
        nb = rng.randint(2, 8)
        slots = [[] for _ in range(nb)]
        for key in range(rng.randint(1, 3 * nb)):
            a, b = rng.sample(range(nb), 2)
            slots[a].append(key); slots[b].append(key)
        layouts = []
        for s in slots:
            rng.shuffle(s)
            pieces = []
            for key in s:
                pieces += [("g", rng.choice((0, 0, 1, thr - 1, thr, thr + 1, 3 * thr))),
                           ("h", rng.choice((1, thr - 1)) if fail and rng.random() < 0.1 else rng.randint(thr, thr + 40), key)]
            pieces.append(("g", rng.choice((0, 1, thr - 1, thr, 50))))
            layouts.append(pieces)
        depths = [rng.choice((1, 1, 2, 3)) for _ in range(nb)]
        alphabet = rng.choice(("ACGT", "ACGTN", "ACGTNRYn"))
        cons = [letters(rng, sum(p[1] for p in pieces), alphabet) for pieces in layouts]
        L.group(layouts, depths=depths, consensus=cons)
    return L.level()


def edit_from_json(e):
    return {"subs": [tuple(x) for x in e["subs"]], "dels": [tuple(x) for x in e["dels"]], "inss": [tuple(x) for x in e["inss"]]}


def reference_graph(vec):
    """the graph and the alignments of test_reweave (reweave.rs:886-1003) from tests/golden/reweave_vectors.json, in the shape of
    simplify.normalize(); the consensus letters are not the reference's (it draws them at random): no expectation reads them"""
    import reweave_ref as rr
    v, w = vec["reweave"], vec["reweave_graph"]
    g = {"paths": {int(p): {"nodes": list(ns), "tot_len": tot, "circular": True, "name": None} for p, (ns, tot) in w["paths"].items()},
         "nodes": {int(n): {"block_id": b, "path_id": p, "strand": s, "position": tuple(pos)} for n, (b, p, s, pos) in w["nodes"].items()}, "blocks": {}}
    for b, (ln, depth) in v["blocks"].items():
        g["blocks"][int(b)] = {"consensus": ("ACGT" * ln)[:ln], "alignments": {n: edit_from_json(w["edits"][str(n)]) for n, x in g["nodes"].items() if x["block_id"] == int(b)}}
        assert len(g["blocks"][int(b)]["alignments"]) == depth
    matches = [{"qry": a["qry"]["name"], "ref": a["reff"]["name"], "qry_start": a["qry"]["start"], "qry_end": a["qry"]["end"], "ref_start": a["reff"]["start"],
                "ref_end": a["reff"]["end"], "reverse": a["reverse"], "cigar": rr.parse_cigar(a["cigar"])} for a in v["alignments"]]
    return g, matches
