"""Batches of block concatenations for the tests of pga_merge_blocks, in the shape pangraph_amd.simplify.merge_blocks takes: blocks =
[{"consensus", "members": [edit]}], edges = [{"left", "right", "left_rc", "right_rc", "partner"}].  What the GPU tests rely on them for is
asserted by tests/test_simplify_cpu.py with the restatement tests/simplify_ref.py alone."""
import random

import simplify_ref as sr

CONS_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 4097)
LIST_LENGTHS = (0, 1, 63, 64, 65, 130)
INS_LENGTHS = (1, 15, 16, 17, 40)
RC = ((False, False), (False, True), (True, False), (True, True))


def _letters(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _increasing(rng, n, hi):
    """n distinct positions in [0, hi], ascending"""
    return sorted(rng.sample(range(hi + 1), n))


def _sorted_member(rng, L, n_sub, n_del, n_ins, ins_len=None):
    """strictly increasing lists of the given lengths (as a graph built by the product holds them)"""
    return {"subs": [(p, rng.choice("ACGT")) for p in _increasing(rng, n_sub, L - 1)] if L else [],
            "dels": [(p, rng.randint(0, min(3, L - p))) for p in _increasing(rng, n_del, L - 1)] if L else [],
            "inss": [(p, _letters(rng, ins_len if ins_len is not None else rng.choice(INS_LENGTHS))) for p in _increasing(rng, n_ins, L)]}


def edge_batch():
    """the sizes at which the kernels take another path (see the asserts in test_simplify_cpu.py)"""
    rng = random.Random(7)
    blocks, edges = [], []

    def add(cons_len, members):
        blocks.append({"consensus": _letters(rng, cons_len), "members": members})
        return len(blocks) - 1

    def join(l, r, rc, partner=None):
        edges.append({"left": l, "right": r, "left_rc": rc[0], "right_rc": rc[1], "partner": list(partner if partner is not None else range(len(blocks[l]["members"])))})

    # every consensus length, depth 1, an insertion at each end: a boundary merge under every strand combination
    small = []
    for k, L in enumerate(CONS_LENGTHS):
        m = _sorted_member(rng, L, min(L, 2), min(L, 1), 0)
        m["inss"] = [(0, _letters(rng, INS_LENGTHS[k % 5]))] + ([(L, _letters(rng, INS_LENGTHS[(k + 2) % 5]))] if L else [])
        small.append(add(L, [m]))
    for k in range(len(small)):
        join(small[k], small[(k + 1) % len(small)], RC[k % 4])
        join(small[(k + 3) % len(small)], small[k], RC[(k + 1) % 4])
    # every list length of every kind, on a long consensus; the partner reverses the members
    wide = [add(4097, [_sorted_member(rng, 4097, n if kind == 0 else 3, n if kind == 1 else 3, n if kind == 2 else 3) for kind in range(3) for n in LIST_LENGTHS]) for _ in range(2)]
    depth = len(blocks[wide[0]]["members"])
    for rc in RC:
        join(wide[0], wide[1], rc, reversed(range(depth)))
    join(wide[1], wide[0], (True, False), [(k + 5) % depth for k in range(depth)])
    # depth 70
    deep = [add(L, [_sorted_member(rng, L, rng.randint(0, 4), rng.randint(0, 3), rng.randint(0, 4)) for _ in range(70)]) for L in (33, 17)]
    join(deep[0], deep[1], (True, False), [(k * 3 + 1) % 70 for k in range(70)])
    join(deep[1], deep[0], (False, True), [(k + 69) % 70 for k in range(70)])
    # list order: two right insertions at one position, equal positions inside a left list, unsorted lists (under *_rc the stable order shows)
    odd = [{"subs": [(9, "A"), (2, "C"), (9, "G"), (5, "T")], "dels": [(9, 2), (2, 5), (9, 0), (3, 1)], "inss": [(5, "AC"), (5, "G"), (3, "TT"), (5, "CAT")]},
           {"subs": [(4, "A"), (4, "C")], "dels": [(4, 1), (4, 2)], "inss": [(4, "AAA"), (4, "C"), (12, "GG"), (12, "T"), (0, "AT"), (0, "G")]},
           {"subs": [], "dels": [(0, 12)], "inss": [(12, "A"), (0, "C"), (12, "G"), (0, "T"), (7, "")]}]
    q = [add(12, [dict(m) for m in odd]), add(12, [dict(m) for m in reversed(odd)])]
    for rc in RC:
        join(q[0], q[1], rc, [1, 2, 0])
        join(q[1], q[0], rc, [0, 1, 2])
        join(q[0], q[0], rc, [2, 0, 1])
    # nothing at all
    empty = [add(0, []), add(5, [])]
    join(empty[0], empty[1], (True, True))
    join(empty[0], empty[0], (False, False))
    return blocks, edges


def _random_member(rng, L):
    def positions(n, hi):
        style = rng.choice((0, 0, 0, 1, 2))
        if style == 0 and n <= hi + 1:
            return _increasing(rng, n, hi)
        p = [rng.randint(0, hi) for _ in range(n)]
        return p if style == 2 else sorted(p)
    n = lambda: rng.choice((0, 0, 1, 2, 3, 6, 70))
    m = {"subs": [], "dels": [], "inss": []}
    if L:
        m["subs"] = [(p, rng.choice("ACGTN")) for p in positions(n(), L - 1)]
        m["dels"] = [(p, rng.randint(0, L - p)) for p in positions(n(), L - 1)]
    m["inss"] = [(p, _letters(rng, rng.choice((0, 1, 2, 15, 16, 17, 40)))) for p in positions(n(), L)]
    if rng.random() < 0.35:
        m["inss"].insert(0, (0, _letters(rng, rng.randint(1, 20))))
    if rng.random() < 0.35:
        m["inss"].append((L, _letters(rng, rng.randint(1, 20))))
    return m


def random_batch(seed):
    """1-8 edges over 2-10 blocks; a few letters have no complement (a lower-case letter or an X)"""
    rng = random.Random(1000 + seed)
    n_blocks = rng.randint(2, 10)
    depth = rng.choice((1, 2, 3, 5))
    blocks = []
    for _ in range(n_blocks):
        L = rng.choice((0, 1, 7, 16, 33, 100, 257))
        blk = {"consensus": _letters(rng, L), "members": [_random_member(rng, L) for _ in range(depth)]}
        if rng.random() < 0.12:
            where = rng.choice(("cons", "ins", "sub"))
            if where == "cons" and L:
                k = rng.randrange(L)
                blk["consensus"] = blk["consensus"][:k] + rng.choice("aX") + blk["consensus"][k + 1:]
            elif where == "ins":
                blk["members"][0]["inss"].append((rng.randint(0, L), "AC" + rng.choice("gX")))
            elif L:
                blk["members"][-1]["subs"].append((rng.randrange(L), rng.choice("tX")))
        blocks.append(blk)
    edges = []
    for k in range(rng.randint(1, 8)):
        rc = RC[(seed + k) % 4]
        perm = list(range(depth))
        rng.shuffle(perm)
        edges.append({"left": rng.randrange(n_blocks), "right": rng.randrange(n_blocks), "left_rc": rc[0], "right_rc": rc[1], "partner": perm})
    return blocks, edges


def batch_facts(blocks, edges):
    """by the restatement alone: per edge its status, the number of boundary merges, and the number of lists that *_rc re-sorts into
    something other than the reversed list"""
    status = [r["status"] for r in sr.merge_batch(blocks, edges)]
    boundary = unsorted = 0
    for e in edges:
        bl, br = blocks[e["left"]], blocks[e["right"]]
        Ll, Lr = len(bl["consensus"]), len(br["consensus"])
        for k, ml in enumerate(bl["members"]):
            mr = br["members"][e["partner"][k]]
            at_end = any((Ll - p if e["left_rc"] else p) == Ll for p, _ in ml["inss"])
            at_start = any((Lr - p if e["right_rc"] else p) == 0 for p, _ in mr["inss"])
            boundary += at_end and at_start
        for blk, rc in ((bl, e["left_rc"]), (br, e["right_rc"])):
            if rc:
                L = len(blk["consensus"])
                for m in blk["members"]:
                    for keys in ([L - p - 1 for p, _ in m["subs"]], [L - p - l for p, l in m["dels"]], [L - p for p, _ in m["inss"]]):
                        unsorted += any(a <= b for a, b in zip(keys, keys[1:]))
    return status, boundary, unsorted


def recon_input(g):
    """a simplified graph -> (blocks, paths, names) as reconstruct takes them"""
    bids = sorted(g["blocks"])
    member_at, blocks = {}, []
    for i, b in enumerate(bids):
        nids = sorted(g["blocks"][b]["alignments"])
        member_at.update({n: (i, j) for j, n in enumerate(nids)})
        blocks.append({"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in nids]})
    paths = [{"nodes": [member_at[n] + (g["nodes"][n]["strand"] == "-",) for n in p["nodes"]], "tot_len": p["tot_len"], "first_pos": g["nodes"][p["nodes"][0]]["position"][0]}
             for _, p in sorted(g["paths"].items())]
    return blocks, paths, [p["name"] for _, p in sorted(g["paths"].items())]
