"""Batches for the minimizer-level tap pga_stage_seed (tests/seedbind.py): generators that aim at the edges of the index build, mid_occ, the query
filter, seed selection, anchor arithmetic and the anchor sort, each with PINS -- what the case was built to hit, stated from the reference's
arithmetic.  tests/test_seed_cases_cpu.py asserts every pin on the reference's own code; tests/test_gpu_seed.py compares the device with it.

Pins (all optional): raw / mid_occ: per group; counts: {sequence: (dropped, used, filtered)} minimizer states; used: {sequence: minimizer indices
used}; tandem: {sequence: seeds with the tandem bit}; rep_len, n_anchors, n_self, n_rev: {sequence: value}; tie: sequences that hold equal anchor
keys (exactly these); routes: route counters of one mode-0 call.

Unless a case says otherwise mid_occ is EXPLICIT and small (2 or 3), so that a "high-occurrence" seed needs three or four copies, not fifty.
"""
import numpy as np

from seedbind import Batch, minimizers, MM_F_NO_DIAG, MM_F_NO_DUAL, MM_F_FOR_ONLY, MM_F_REV_ONLY, MO_BINS, MO_KEYS

PROD = MM_F_NO_DIAG | MM_F_NO_DUAL


class Bld:
    """one batch under construction: sequences, groups, minimizers put at explicit positions or at the next free one"""

    def __init__(self, k=15, w=10, **params):
        self.k, self.w = k, w
        self.params = dict(k=k, w=w, **params)
        self.lens, self.names, self.recs, self.cur, self.grp_off = [], [], [], [], [0]
        self.next_hash = 1

    def seq(self, length=None, name=None):
        self.lens.append(length)
        self.names.append(name if name is not None else str(len(self.lens) - 1).encode())
        self.recs.append([])
        self.cur.append(self.k - 1)
        return len(self.lens) - 1

    def group(self):
        """close the current group; the next sequence opens a new one"""
        self.grp_off.append(len(self.lens))

    def fresh(self):
        self.next_hash += 1
        return self.next_hash

    def put(self, s, pos, h, strand=0):
        self.recs[s].append((h, pos, strand))
        self.cur[s] = max(self.cur[s], pos + 1)
        return len(self.recs[s]) - 1

    def add(self, s, h, strand=0, gap=1):
        """at the next free position of sequence s"""
        pos = self.cur[s] + gap - 1
        self.put(s, pos, h, strand)
        return pos

    def spread(self, seqs, h, count, strand=0, gap=1):
        for c in range(count):
            self.add(seqs[c % len(seqs)], h, strand if strand in (0, 1) else c & 1, gap)

    def singles(self, s, n, gap=1):
        for _ in range(n):
            self.add(s, self.fresh(), 0, gap)

    def batch(self, name, own=None, **pins):
        if self.grp_off[-1] != len(self.lens):
            self.grp_off.append(len(self.lens))
        mz, lens = [], []
        for s, recs in enumerate(self.recs):
            recs = sorted(recs, key=lambda r: r[1])
            pos = [r[1] for r in recs]
            assert all(a < b for a, b in zip(pos, pos[1:])), (name, s, "positions collide")
            L = self.lens[s] if self.lens[s] is not None else (pos[-1] + 1 + 3 if pos else self.k + 3)
            assert not pos or (pos[0] >= self.k - 1 and pos[-1] < L), (name, s)
            assert all(0 < r[0] < 1 << 2 * self.k for r in recs)
            lens.append(L)
            mz.append(minimizers(self.k, s, recs))
        return Batch(name, lens, list(self.names), list(self.grp_off), mz, dict(self.params), own, pins)


def ref_index_kk(n, f=np.float32(2e-4)):
    """(uint32)((1. - f) * n) as index.c:204 computes it: double arithmetic on the float fraction"""
    return int((1. - float(np.float32(f))) * n)


# ---------------------------------------------------------------- mid_occ
def _counts_batch(name, groups, params=None, probe=True, **pins):
    """groups: per group a list of occurrence counts, one per key (hash order = list order).  Every group gets two target sequences that
    hold the copies and are not mapped (own = 0: a key with thousands of copies is never expanded into anchors on both sides), and a mapped probe
    sequence with three singletons and one copy of the group's first key."""
    b = Bld(15, 10, **{**dict(mid_occ=0, max_mid_occ=100000, min_mid_occ=1, flag=MM_F_NO_DIAG), **(params or {})})
    own = []
    for counts in groups:
        t = [b.seq(), b.seq()]
        q = b.seq()
        own += [0, 0, 1]
        h0 = b.next_hash + 1
        for c in counts:
            b.spread(t, b.fresh(), c)
        if probe and counts:
            b.add(q, h0)                                   # one more copy of the first key
            b.singles(q, 3)
        b.group()
    return b.batch(name, own=own, **pins)


def _keys(n_keys, top):
    """n_keys counts: `top` (distinct, descending) and ones, minus the probe's additions: the probe adds one copy to the first key and three
    singleton keys"""
    return [top[0] - 1] + list(top[1:]) + [1] * (n_keys - len(top) - 3)


def mid_occ_cases():
    out = []
    top = [60, 58, 56, 54]
    for n in (4999, 5000, 5001, 9999, 10000, 10001, 15000, 15001):
        kk = ref_index_kk(n)
        rank = n - 1 - kk                                  # 0: the largest count answers
        assert rank == (0 if n <= 5000 else 1 if n <= 10000 else 2 if n <= 15000 else 3), (n, kk)
        out.append(_counts_batch(f"mid_occ/n_keys={n}", [_keys(n, top)], raw=[top[rank] + 1], mid_occ=[top[rank] + 1], routes=dict(mo_hist=1, mo_sort=0)))
    # the histogram's last bin collects every count >= MO_BINS - 1 = 1023: an ANSWER there (raw >= 1024) sends the batch to the sort
    for raw in (1021, 1022, 1023, 1024, 5000):
        sort = raw - 1 >= MO_BINS - 1
        out.append(_counts_batch(f"mid_occ/raw={raw}", [_keys(40, [raw - 1, 7])], raw=[raw], mid_occ=[raw], routes=dict(mo_hist=int(not sort), mo_sort=int(sort))))
    out.append(_counts_batch("mid_occ/big_count_above_answer", [_keys(5001, [2000, 30])], raw=[31], routes=dict(mo_hist=1, mo_sort=0)))
    out.append(_counts_batch("mid_occ/resolved_and_unresolved", [_keys(50, [12, 3]), _keys(60, [3000, 9])], raw=[13, 3001], routes=dict(mo_hist=0, mo_sort=1)))
    for raw, lo, hi, want in ((49, 50, 500, 50), (50, 50, 500, 50), (51, 50, 500, 51), (499, 50, 500, 499), (500, 50, 500, 500), (501, 50, 500, 500),
                              (600, 50, 40, 600), (600, 50, 50, 600), (30, 50, 40, 50)):
        out.append(_counts_batch(f"mid_occ/clamp raw={raw} min={lo} max={hi}", [_keys(30, [raw - 1, 5])], dict(min_mid_occ=lo, max_mid_occ=hi), raw=[raw], mid_occ=[want]))
    out.append(_counts_batch("mid_occ/empty_group", [_keys(20, [9, 4]), [], _keys(25, [6, 2])], dict(min_mid_occ=0), raw=[10, 1, 7], mid_occ=[10, 1, 7]))
    out.append(_counts_batch("mid_occ/empty_group_clamped", [[], _keys(25, [6, 2])], dict(min_mid_occ=50, max_mid_occ=500), raw=[1, 7], mid_occ=[50, 50]))
    # group boundaries at the edge of a k_mo_hist workgroup (MO_KEYS keys): the first group holds exactly that many keys
    for n0 in (MO_KEYS - 1, MO_KEYS, MO_KEYS + 1):
        out.append(_counts_batch(f"mid_occ/boundary_at_key={n0}", [_keys(n0, [17, 5]), _keys(300, [23, 4]), _keys(MO_KEYS + 5, [11, 2])], raw=[18, 24, 12]))
    # a workgroup whose first key belongs to group 0 and all its other keys to group 1, and one that starts inside a tiny group
    out.append(_counts_batch("mid_occ/first_key_of_another_group", [_keys(MO_KEYS + 1, [8, 5]), _keys(1500, [9, 4])], raw=[9, 10]))
    out.append(_counts_batch("mid_occ/tiny_groups_in_one_workgroup", [_keys(6, [4, 2]), _keys(7, [3, 2]), _keys(2 * MO_KEYS + 3, [14, 3]), _keys(5, [5])], raw=[5, 4, 15, 6]))
    out.append(_counts_batch("mid_occ/explicit", [_keys(40, [30, 7]), _keys(40, [90, 7])], dict(mid_occ=7), mid_occ=[7, 7], routes=dict(mo_hist=0, mo_sort=0)))
    return out


# ---------------------------------------------------------------- the query filter (seed.c:5-28)
def _flt_batch(name, copies, n_mv, mid_occ, frac=0.01, others=None, **pins):
    """one group: query 0 with n_mv minimizers, of which copies[i] carry key i (spread evenly, never neighbours); a second sequence with
    `others` = {key index: copies} and singletons"""
    b = Bld(15, 10, mid_occ=mid_occ, q_occ_frac=frac, occ_dist=0, max_max_occ=100000)
    q, t = b.seq(), b.seq()
    hs = [b.fresh() for _ in copies]
    slots = [None] * n_mv
    for i, c in enumerate(copies):
        step = max(n_mv // c, 1) if c else 1
        j = i
        for _ in range(c):
            while slots[j % n_mv] is not None:
                j += 1
            slots[j % n_mv] = hs[i]
            j += step
    for s in slots:
        b.add(q, s if s is not None else b.fresh(), 0, 2)
    for i, c in (others or {}).items():
        b.spread([t], hs[i], c, gap=2)
    b.singles(t, 4)
    return b.batch(name, **pins)


def query_filter_cases():
    out = []
    f32 = np.float32
    # n_mv against mid_occ: the filter is not entered with n_mv <= mid_occ (seed.c:9)
    out.append(_flt_batch("flt/n_mv=mid_occ", [6], 6, 6, counts={0: (0, 6, 0)}))
    out.append(_flt_batch("flt/n_mv=mid_occ+1", [7], 7, 6, counts={0: (7, 0, 0)}))
    # copies inside the query against mid_occ
    out.append(_flt_batch("flt/copies=mid_occ", [5], 100, 5, counts={0: (0, 100, 0)}))
    out.append(_flt_batch("flt/copies=mid_occ+1", [6], 100, 5, counts={0: (6, 94, 0)}))
    # copies against n_mv * q_occ_frac, compared in float
    for n_mv in (300, 700, 1100, 1500, 1900, 650):
        prod = f32(n_mv) * f32(0.01)
        for c in (n_mv // 100, n_mv // 100 + 1):
            drop = bool(f32(c) > prod)
            out.append(_flt_batch(f"flt/frac n_mv={n_mv} copies={c}", [c], n_mv, 2, counts={0: (c, n_mv - c, 0) if drop else (0, n_mv - c, c)}))
    out.append(_flt_batch("flt/frac=0", [40], 100, 5, frac=0.0, counts={0: (0, 60, 40)}))
    out.append(_flt_batch("flt/frequent_in_group_only", [1], 100, 5, others={0: 50}, counts={0: (0, 99, 1)}))
    out.append(_flt_batch("flt/two_keys", [9, 7, 5], 120, 5, counts={0: (16, 104, 0)}))
    out.append(_flt_batch("flt/query_loses_all", [30, 30], 60, 5, counts={0: (60, 0, 0)}, n_anchors={0: 0}))
    # a batch that loses every minimizer: both sequences hold nothing but one over-represented key each
    b = Bld(15, 10, mid_occ=3, occ_dist=0, max_max_occ=100000)
    for _ in range(2):
        s = b.seq()
        b.spread([s], b.fresh(), 20, gap=2)
    out.append(b.batch("flt/batch_loses_all", counts={0: (20, 0, 0), 1: (20, 0, 0)}, n_anchors={0: 0, 1: 0}))
    # ... and one that loses none (no compaction: kept_idx stays null)
    b = Bld(15, 10, mid_occ=3, occ_dist=0, max_max_occ=100000)
    a, c = b.seq(), b.seq()
    for _ in range(30):
        h = b.fresh()
        b.add(a, h, 0, 2)
        b.add(c, h, 1, 3)
    out.append(b.batch("flt/batch_loses_none", counts={0: (0, 30, 0), 1: (0, 30, 0)}))
    return out


# ---------------------------------------------------------------- seed selection (seed.c:56-131)
def _sel(name, seeds, qlen=None, mid_occ=2, params=None, **pins):
    """one group: query 0 with `seeds` = [(position, occurrence count in the group)], every seed a key of its own; sequence 1 holds the other
    count - 1 copies of each key.  A seed is high with count > mid_occ."""
    b = Bld(15, 10, **{**dict(mid_occ=mid_occ, flag=0), **(params or {})})
    q, t = b.seq(qlen), b.seq()
    for pos, cnt in seeds:
        h = b.fresh()
        b.put(q, pos, h)
        b.spread([t], h, cnt - 1)
    return b.batch(name, **pins)


def selection_cases():
    out = []
    H, L = 4, 1        # counts of a high and of a low seed under mid_occ = 2
    # a query with exactly one seed, and that seed high: the quota branch returns at once (seed.c:63); the other branch filters it
    out.append(_sel("sel/one_seed quota", [(100, H)], 400, counts={0: (0, 1, 0)}, rep_len={0: 0}))
    out.append(_sel("sel/one_seed occ_dist=0", [(100, H)], 400, params=dict(occ_dist=0), counts={0: (0, 0, 1)}, rep_len={0: 15}))
    out.append(_sel("sel/one_seed max_max_occ=mid_occ", [(100, H)], 400, params=dict(max_max_occ=2), counts={0: (0, 0, 1)}, rep_len={0: 15}))
    out.append(_sel("sel/one_seed max_max_occ<mid_occ", [(100, H)], 400, params=dict(max_max_occ=1), counts={0: (0, 0, 1)}, rep_len={0: 15}))
    # streak spans pe - ps between two low seeds: (int)(span / 500 + .499) high seeds stay
    for span, quota in ((250, 0), (251, 1), (750, 1), (751, 2), (1250, 2), (1251, 3)):
        p0 = 40
        seeds = [(p0, L)] + [(p0 + 20 + 30 * j, H + j) for j in range(4)] + [(p0 + span, L)]
        out.append(_sel(f"sel/span={span}", seeds, p0 + span + 40, counts={0: (0, 2 + quota, 4 - quota)}, used={0: list(range(0, 1 + quota)) + [5]}))
    # a streak at the query's start (ps = 0) and one at its end (pe = len)
    for first_low, quota in ((250, 0), (251, 1)):
        out.append(_sel(f"sel/streak_at_start pe={first_low}", [(20, H), (60, H + 1), (first_low, L), (first_low + 30, L)], first_low + 100,
                        counts={0: (0, 2 + quota, 2 - quota)}))
    for tail, quota in ((250, 0), (251, 1)):
        out.append(_sel(f"sel/streak_at_end len-ps={tail}", [(30, L), (60, L), (100, H + 1), (140, H)], 60 + tail, counts={0: (0, 2 + quota, 2 - quota)},
                        used={0: [0, 1, 3][:2 + quota]}))
    # streaks separated by a single low seed: each gets its own quota
    out.append(_sel("sel/streaks_one_low_apart", [(20, H), (100, H + 1), (300, L), (400, H + 2), (500, H), (700, L), (720, H)], 800,
                    counts={0: (0, 4, 3)}, used={0: [0, 2, 4, 5]}))
    # more seeds than the quota and equal counts at the heap's top: the earlier index stays, only a strictly smaller count replaces it
    out.append(_sel("sel/heap_ties", [(40, L)] + [(60 + 20 * j, c) for j, c in enumerate([5, 4, 4, 4, 7, 4])] + [(40 + 751, L)], 900,
                    counts={0: (0, 4, 4)}, used={0: [0, 2, 3, 7]}))
    out.append(_sel("sel/heap_ties_three", [(40, L)] + [(60 + 20 * j, c) for j, c in enumerate([6, 6, 6, 5, 6, 5, 5, 9, 3])] + [(40 + 1251, L)], 1400,
                    counts={0: (0, 5, 6)}, used={0: [0, 4, 6, 9, 10]}))
    # 140 high seeds under a quota of 128 (uncapped) and of 129 (capped to 128): the 128 smallest under (count, index) stay
    for span in (64250, 64251):
        rng = np.random.default_rng(span)
        cnts = [int(c) for c in rng.integers(3, 7, 140)]
        seeds = [(40, L)] + [(100 + 450 * j, cnts[j]) for j in range(140)] + [(40 + span, L)]
        order = sorted(range(140), key=lambda j: (cnts[j], j))[:128]
        out.append(_sel(f"sel/span={span} 140_high", seeds, 40 + span + 30, counts={0: (0, 130, 12)}, used={0: [0] + sorted(1 + j for j in order) + [141]}))
    # chosen by the quota and filtered all the same: count above max_max_occ
    for cnt, flt in ((4095, 0), (4096, 1)):
        out.append(_sel(f"sel/max_max_occ count={cnt}", [(40, L), (100, cnt), (40 + 400, L)], 600, counts={0: (0, 3 - flt, flt)}, rep_len={0: 15 * flt}))
    # rep_len: intervals [pos + 1 - k, pos + 1) of filtered seeds merge unless the next one starts beyond the end: closer than k, k apart, k + 1 apart
    k = 15
    seeds = [(40, L), (60, H), (65, H), (65 + k, H), (65 + 2 * k + 1, H), (250, L)]
    out.append(_sel("sel/rep_len", seeds, 300, counts={0: (0, 2, 4)}, rep_len={0: (65 + k + 1 - (60 + 1 - k)) + k}))
    out.append(_sel("sel/rep_len_at_start", [(14, H), (20, H), (200, L), (230, L)], 300, counts={0: (0, 2, 2)}, rep_len={0: 21}))
    return out


# ---------------------------------------------------------------- anchors (map.c:78-100,168-204) and their sort
def _mixed_group(b, n, rng, n_keys=12, per_seq=14, names=None, lens=None):
    """n sequences that share n_keys keys on both strands (a key may lie twice in one sequence), plus singletons"""
    ids = [b.seq(lens[i] if lens else None, names[i] if names else None) for i in range(n)]
    hs = [b.fresh() for _ in range(n_keys)]
    for s in ids:
        for _ in range(per_seq):
            r = rng.random()
            b.add(s, hs[int(rng.integers(n_keys))] if r < 0.7 else b.fresh(), int(rng.integers(2)), int(rng.integers(1, 30)))
    return ids


def anchor_cases():
    out = []
    for flag in (0, MM_F_NO_DIAG, MM_F_NO_DUAL, MM_F_FOR_ONLY, MM_F_REV_ONLY, PROD, PROD | MM_F_FOR_ONLY, PROD | MM_F_REV_ONLY, MM_F_FOR_ONLY | MM_F_REV_ONLY):
        b = Bld(15, 10, mid_occ=1000, flag=flag)
        _mixed_group(b, 3, np.random.default_rng(7))
        pins = dict(n_anchors={0: 0, 1: 0, 2: 0}) if flag == MM_F_FOR_ONLY | MM_F_REV_ONLY else {}
        out.append(b.batch(f"anchor/flag={flag:#x}", **pins))
    # a group of one sequence: only off-diagonal self hits, SEED_SELF on the same strand only
    b = Bld(15, 10, mid_occ=1000, flag=PROD)
    s = b.seq()
    h1, h2 = b.fresh(), b.fresh()
    for pos, h, st in ((20, h1, 0), (50, h2, 0), (90, h1, 0), (130, h2, 1), (170, h1, 1)):
        b.put(s, pos, h, st)
    b.singles(s, 3, 9)
    out.append(b.batch("anchor/group_of_one", n_anchors={0: 8}, n_self={0: 2}, n_rev={0: 6}))
    # names: strcmp order differs from numeric order and from length order; a byte of 0x80 or above compares as unsigned
    names = [b"9", b"10", b"12", b"123", b"\x80z", b"~", b"1"]
    for flag in (PROD, MM_F_NO_DUAL):
        b = Bld(15, 10, mid_occ=1000, flag=flag)
        _mixed_group(b, len(names), np.random.default_rng(11), names=names, lens=[900, 700, 800, 650, 750, 1000, 850])
        out.append(b.batch(f"anchor/names flag={flag:#x}"))
    # a reverse-strand hit of the first possible position (k - 1) and of the last (len - 1), as query and as target
    b = Bld(15, 10, mid_occ=1000, flag=0)
    q, t = b.seq(200), b.seq(300)
    h1, h2 = b.fresh(), b.fresh()
    b.put(q, 14, h1, 0), b.put(q, 199, h2, 1), b.put(t, 14, h2, 0), b.put(t, 299, h1, 1)
    out.append(b.batch("anchor/reverse_first_and_last", n_anchors={0: 4, 1: 4}, n_rev={0: 2, 1: 2}))
    # tandem: neighbouring equal hashes inside a query; the last minimizer of query q and the first of q + 1 are no neighbours
    b = Bld(15, 10, mid_occ=1000, flag=MM_F_NO_DIAG)
    q0, q1, q2 = b.seq(), b.seq(), b.seq()
    h, g = b.fresh(), b.fresh()
    b.singles(q0, 2, 7), b.add(q0, h, 0, 5)                       # q0 ends in h
    b.add(q1, h, 0, 5), b.singles(q1, 2, 7), b.add(q1, g, 0, 4), b.add(q1, g, 1, 4), b.add(q1, g, 0, 4), b.singles(q1, 1, 7), b.add(q1, h, 0, 5)
    b.add(q2, h, 1, 5), b.add(q2, h, 0, 9), b.singles(q2, 2, 7)  # q2 starts with two h
    out.append(b.batch("anchor/tandem", tandem={0: 0, 1: 3, 2: 2}))
    # ... and the same with a query filter in between: neighbours are those of the FILTERED list
    b = Bld(15, 10, mid_occ=3, flag=MM_F_NO_DIAG, q_occ_frac=0.01, occ_dist=0, max_max_occ=100000)
    q0, q1 = b.seq(), b.seq()
    h, g = b.fresh(), b.fresh()
    b.add(q0, h, 0, 3)
    for _ in range(4):
        b.add(q0, g, 0, 3)                                        # g: four copies, over-represented, dropped -> the two h become neighbours
    b.add(q0, h, 1, 3), b.singles(q0, 2, 5)
    b.add(q1, h, 0, 3), b.singles(q1, 3, 5)
    out.append(b.batch("anchor/tandem_across_dropped", counts={0: (4, 4, 0)}, tandem={0: 2, 1: 0}))
    # equal x from two query seeds on one target position: a tie, sent through the replay
    b = Bld(15, 10, mid_occ=1000, flag=PROD)
    q, t = b.seq(None, b"a"), b.seq(None, b"b")
    h, g = b.fresh(), b.fresh()
    b.put(q, 30, h, 0), b.put(q, 80, g, 0), b.put(q, 140, h, 0), b.put(q, 200, g, 1), b.put(q, 260, h, 0)
    b.put(t, 50, h, 0), b.put(t, 120, g, 1), b.singles(t, 2, 9)
    out.append(b.batch("anchor/equal_x_two_seeds", tie=[0], routes=dict(replay_q=1)))
    # queries without anchors first, in the middle and last
    b = Bld(15, 10, mid_occ=1000, flag=PROD)
    s = [b.seq() for _ in range(7)]
    for i in (0, 3, 6):
        b.singles(s[i], 5, 6)
    hs = [b.fresh() for _ in range(5)]
    for i in (1, 2, 4, 5):
        for j, h in enumerate(hs):
            b.add(s[i], h, (i + j) & 1, 8)
    b.add(s[4], b.fresh())
    out.append(b.batch("anchor/empty_queries", n_anchors={0: 0, 3: 0, 6: 0}))
    # two equal x as the last anchor of one query and the first of the next: no tie, no replay.  NO_DUAL maps a query to the names not below
    # its own: "b" (sequence 1) reaches only "c" (sequence 0); "a" (sequence 2) reaches "c" at the same position first, then "b"
    b = Bld(15, 10, mid_occ=1000, flag=PROD)
    t, qa, qb = b.seq(None, b"c"), b.seq(None, b"b"), b.seq(None, b"a")
    h = b.fresh()
    b.put(t, 77, h, 0), b.put(qa, 40, h, 0), b.put(qb, 90, h, 0)
    for s_ in (t, qa, qb):
        b.singles(s_, 2, 11)
    out.append(b.batch("anchor/equal_x_across_queries", n_anchors={0: 0, 1: 1, 2: 2}, tie=[], routes=dict(replay_q=0)))
    # the widths of the packed sort key: position bits from the longest sequence, target bits from the largest group; anchors on the last
    # target at its last position, both strands (the strand bit lies above both)
    for n in (2, 3, 256, 257):
        for L in (65535, 65536, 65537):
            b = Bld(15, 10, mid_occ=1000, flag=0)
            ids = [b.seq() for _ in range(n - 1)] + [b.seq(L)]
            h, g = b.fresh(), b.fresh()
            b.put(ids[0], 30, h, 0), b.put(ids[0], 60, g, 1), b.put(ids[0], 90, h, 0)
            for s_ in ids[1:-1]:
                b.singles(s_, 1)
            if n > 2:
                b.put(ids[n - 2], 40, g, 0)
            b.put(ids[-1], 20, g, 0), b.put(ids[-1], L - 2, h, 1), b.put(ids[-1], L - 1, h, 0)
            out.append(b.batch(f"anchor/key_width n={n} len={L}"))
    # three groups in a batch with the same hashes in each: ids relative to the group, lists apart
    b = Bld(15, 10, mid_occ=1000, flag=PROD)
    for gi in range(3):
        b.next_hash = 1
        _mixed_group(b, 2 + gi, np.random.default_rng(3 + gi), n_keys=6)
        b.group()
    out.append(b.batch("anchor/three_groups_same_hashes"))
    # 300 groups of tiny sequences at k = 28: 56 hash bits and 9 group bits do not fit one sort key
    b = Bld(28, 10, mid_occ=1000, flag=PROD)
    rng = np.random.default_rng(28)
    for gi in range(300):
        ids = [b.seq() for _ in range(2 + gi % 2)]
        hs = [int(rng.integers(1, 1 << 56)) | (gi & 1) << 55 for _ in range(3)] + [(1 << 56) - 1, 1]
        for s_ in ids:
            for h in hs:
                if rng.random() < 0.8:
                    b.add(s_, h, int(rng.integers(2)), int(rng.integers(1, 9)))
        b.group()
    out.append(b.batch("anchor/300_groups_k=28", routes=dict(idx_one_sort=0, idx_two_sorts=1)))
    # an own mask that leaves out a query whose minimizers stay targets
    b = Bld(15, 10, mid_occ=1000, flag=MM_F_NO_DIAG)
    _mixed_group(b, 4, np.random.default_rng(5))
    out.append(b.batch("anchor/own_mask", own=[1, 0, 1, 0], n_anchors={1: 0, 3: 0}, counts={1: (14, 0, 0), 3: (14, 0, 0)}))
    b = Bld(15, 10, mid_occ=1000, flag=MM_F_NO_DIAG)
    _mixed_group(b, 3, np.random.default_rng(6))
    out.append(b.batch("anchor/own_mask_none_mapped", own=[0, 0, 0], n_anchors={0: 0, 1: 0, 2: 0}))
    return out


def random_cases():
    """forty seeded batches of one to five groups; mid_occ is DERIVED with clamps of [3, 8] and the count distributions are drawn to cross it"""
    out = []
    for seed in range(40):
        rng = np.random.default_rng(1000 + seed)
        k = int(rng.choice([11, 15, 19, 21]))
        b = Bld(k, 10, mid_occ=0, min_mid_occ=3, max_mid_occ=int(rng.choice([8, 8, 2])), occ_dist=int(rng.choice([500, 100, 0])),
                max_max_occ=int(rng.choice([4095, 12, 2])), q_occ_frac=float(rng.choice([0.01, 0.05, 0.0])),
                flag=int(rng.choice([PROD, PROD, 0, MM_F_NO_DIAG, PROD | MM_F_FOR_ONLY])))
        for _ in range(int(rng.integers(1, 6))):
            n = int(rng.integers(1, 5))
            ids = [b.seq() for _ in range(n)]
            keys = [(b.fresh(), int(c)) for c in np.minimum(rng.geometric(0.25, int(rng.integers(5, 60))), 30)]
            recs = [h for h, c in keys for _ in range(c)]
            rng.shuffle(recs)
            for h in recs:
                b.add(ids[int(rng.integers(n))], h, int(rng.integers(2)), int(rng.choice([1, 1, 2, 7, 40, 300])))
            b.group()
        out.append(b.batch(f"random/{seed}"))
    return out


FAMILIES = {"mid_occ": mid_occ_cases, "query_filter": query_filter_cases, "selection": selection_cases, "anchors": anchor_cases, "random": random_cases}
_CACHE = {}


def family(name):
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
    return _CACHE[name]
