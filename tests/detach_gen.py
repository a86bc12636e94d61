"""Batches for the tests of pga_detach_unaligned: blocks = [{"consensus", "members": [edit]}], who = per block [(node_id, reverse)].
edge_batch(): the smallest shapes at which the kernels can go wrong; random_batch(seed): up to 30 blocks x 12 members over at most 300
letters, about a quarter of the members unaligned; status_batch(): a rejected complement, a literal '-' and a good orphan side by side."""
import random

import detach_ref as dr

ORPHAN_LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 4097)      # the unit edges of k_rows; the hash message is 16 + len bytes: stripes and tails
LIST_LENGTHS = (0, 1, 63, 64, 65, 130)                                 # across the lane stride


def _letters(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _kept(rng, L, n):
    """n entries in each list; the deletions are single letters, so that their sum stays under L"""
    assert n < L or n == 0
    return {"subs": [((2 * t) % L, "ACGT"[t & 3]) for t in range(n)], "dels": [(t % L, 1) for t in range(n)], "inss": [(t % (L + 1), _letters(rng, 1 + t % 3)) for t in range(n)]}


def _orphan(rng, L, n, pos):
    return {"subs": [], "dels": [(0, L)] if L else [], "inss": [(pos, _letters(rng, n))] if n else []}


class _Batch:
    def __init__(self, rng):
        self.rng, self.blocks, self.who, self.next_id = rng, [], [], 1

    def block(self, L, members, reverse=None):
        self.blocks.append({"consensus": _letters(self.rng, L), "members": members})
        w = []
        for k in range(len(members)):
            w.append((self.next_id, bool(self.rng.randrange(2)) if reverse is None else bool(reverse[k])))
            self.next_id += 1 + self.rng.randrange(1 << 40)
        self.who.append(w)


def edge_batch():
    rng = random.Random(20260412)
    B = _Batch(rng)
    B.block(20, [_orphan(rng, 20, 5, 0), _kept(rng, 20, 0), _kept(rng, 20, 1)], [0, 1, 0])                                  # the first member
    B.block(20, [_kept(rng, 20, 2), _kept(rng, 20, 0), _orphan(rng, 20, 7, 20)], [0, 0, 1])                                 # the last
    B.block(9, [_orphan(rng, 9, 3, 4), _orphan(rng, 9, 0, 0), _orphan(rng, 9, 2, 9)], [0, 1, 1])                            # all of them
    B.block(33, [_kept(rng, 33, 3), _orphan(rng, 33, 1, 0), _orphan(rng, 33, 1, 33), _kept(rng, 33, 1)], [1, 1, 0, 0])      # two neighbours
    B.block(12, [])                                                                                                        # no member
    B.block(0, [_orphan(rng, 0, 0, 0), _orphan(rng, 0, 6, 0), _orphan(rng, 0, 0, 0)], [0, 1, 1])                            # cons_len == 0, with and without insertions
    B.block(40, [{"subs": [], "dels": [(0, 20), (20, 20)], "inss": []},                                                    # the sum equals cons_len
                 {"subs": [], "dels": [(0, 20), (20, 19)], "inss": []},                                                    # cons_len - 1: kept
                 {"subs": [(30, "T"), (3, "G")], "dels": [(0, 20), (5, 15), (0, 5)], "inss": []}], [0, 1, 1])              # the sum, not the union
    B.block(300, [_kept(rng, 300, n) for n in LIST_LENGTHS])
    B.block(200, [_kept(rng, 200, 5), {"subs": [], "dels": [(t, 1) for t in range(200)], "inss": [(100, _letters(rng, 21))]}], [0, 1])   # 200 deletions that tile
    members, reverse = [], []
    for n in ORPHAN_LENGTHS:
        for rev in (0, 1):
            members.append(_orphan(rng, 64, n, (0, 31, 64)[len(members) % 3])); reverse.append(rev)
    B.block(64, members, reverse)
    B.block(50, [{"subs": [], "dels": [(0, 50)], "inss": [(50, "ACGTT"), (0, "GGA"), (25, "TTTTTTTTTTTTTTTTTTC"), (25, "AC"), (0, "")]}, _kept(rng, 50, 4)], [1, 0])   # several insertions
    return B.blocks, B.who


def random_batch(seed):
    rng = random.Random(7000 + seed)
    B = _Batch(rng)
    n_blocks = rng.randint(6, 30)
    emptied = rng.randrange(1, n_blocks)                                      # every member of this block is unaligned, a forward and a reverse one among them
    for b in range(n_blocks):
        L = rng.choice((0, 1, 15, 16, 17, 33, 100, 300)) if b and rng.random() < 0.5 else rng.randint(1, 300)
        depth = rng.randint(0 if b != emptied else 2, 12)
        members = [{"subs": [], "dels": [], "inss": []}] if b == 0 else []      # (block 0 has a consensus and a member without edits: kept)
        for _ in range(depth):
            e = {"subs": [(rng.randrange(L), rng.choice("ACGTN")) for _ in range(rng.choice((0, 1, 3, 70)))] if L else [],
                 "dels": [], "inss": [(rng.randint(0, L), _letters(rng, rng.choice((0, 1, 5, 16, 40)))) for _ in range(rng.choice((0, 0, 1, 2, 5)))]}
            if L:
                for _ in range(rng.choice((0, 1, 2, 66 if L >= 150 else 3))):  # (short ones: their sum stays under a long consensus)
                    p = rng.randrange(L)
                    e["dels"].append((p, rng.randint(0, min(L - p, 2))))
                if b == emptied or rng.random() < 0.15:                         # unaligned: one deletion over everything, or two that meet
                    cut = rng.randint(0, L)
                    e["dels"] += [(0, L)] if rng.random() < 0.5 else [(cut, L - cut), (0, cut)]
                    rng.shuffle(e["dels"])
            members.append(e)
        B.block(L, members[:12], [False, True] + [rng.randrange(2) for _ in members[2:]] if b == emptied else None)
    return B.blocks, B.who


def status_batch():
    rng = random.Random(5)
    B = _Batch(rng)
    B.block(24, [{"subs": [], "dels": [(0, 24)], "inss": [(0, "ACGTaCGT")]},                # reverse, a lower-case letter: 2
                 {"subs": [], "dels": [(0, 24)], "inss": [(24, "ACG-T")]},                  # a literal '-': 3
                 {"subs": [], "dels": [(0, 24)], "inss": [(12, "ACGTTGCA")]},               # good
                 {"subs": [], "dels": [(0, 24)], "inss": [(0, "ACGTaCGT")]},                # forward: its letters are not checked
                 _kept(rng, 24, 2)], [1, 0, 1, 0, 1])
    B.block(16, [_kept(rng, 16, 1), {"subs": [(10, "-")], "dels": [(0, 8), (0, 8)], "inss": []}], [0, 1])   # a substituted '-' that no deletion hides: 3
    return B.blocks, B.who


def batch_facts(blocks, who):
    """-> (kept, forward orphans, reverse orphans, blocks emptied) of a batch"""
    kept = fwd = rev = emptied = 0
    for b, w in zip(blocks, who):
        un = [dr.aligned_count(e, len(b["consensus"])) == 0 for e in b["members"]]
        kept += un.count(False)
        fwd += sum(1 for u, (_, r) in zip(un, w) if u and not r)
        rev += sum(1 for u, (_, r) in zip(un, w) if u and r)
        emptied += bool(un) and all(un)
    return kept, fwd, rev, emptied
