"""Cases for the region planner (pga_plan.hip), built against its kernels: 64-lane windows whose first lane takes a carried predecessor, trips of
eight windows, ballot / n-th-bit selection with a count carried across windows, the capped LDS list of long gaps, several cuts in one window,
runs open across windows of segments, the zero-copy and the device-copy host route.

A case is a planbind.Group: a few sequences, a query's anchors, regions and parameters.  Every group starts with a short sequence outside the
group (base = 1), so that no query or target lies at offset 0 of the store and the group does not start at sequence 0.  Each case carries PINS:
what it was built to hit, stated as values the reference must produce (tests/test_plan_cases_cpu.py asserts them on the reference alone):

  out      {(region, field): value}      fields of planbind.OUT_FIELDS
  ignore   {region: set of chain indices (relative to as) flagged MM_SEED_IGNORE by this region's plan}
  join     {region: set of chain indices flagged MM_SEED_LONG_JOIN by this region's plan}
  segs     {region: number of gap-fill segments}
  items    {region: [(kind, bw1, m), ...]}

Notes on what anchors cannot express: rs1 clamped at 0 cannot be told from an unclamped negative rs1, since rs1 only bounds max(rs1, rs - l) from
below and rs - l >= 0; a burst's weight is ins + del - |ins - del| = 2 min(ins, del), always even, so the pair
around the threshold 40 is 40 / 42; qe = qlen and re = tlen need an anchor at position len + k/2, outside its sequence, which the tap refuses.
"""
import numpy as np

import planbind as pb
from planbind import A_IGNORE, A_LONG_JOIN, A_SELF, A_TANDEM, Group, revcomp

SPAN, HALF_K = 15, 7
_DUMMY = np.array([0, 1, 4, 2, 3, 3, 1, 0, 4, 2] * 3 + [1, 2, 3, 0, 1, 2, 3], np.uint8)      # 37 bases: what follows sits at an odd offset


class Builder:
    """one query against a few targets"""

    def __init__(self, name, tlens, qlen, seed=1, base=1, **params):
        self.name, self.params, self.base = name, params, base
        self.rng = np.random.default_rng(seed)
        self.targets = [self.rng.integers(0, 4, n).astype(np.uint8) for n in tlens]
        self.q = self.rng.integers(0, 4, qlen).astype(np.uint8)          # forward strand; unrelated to the targets until a chain is laid
        self.anchors, self.regions, self.pins = [], [], {}
        self.laid = []

    # -- anchors
    def chain(self, rev, rid, t0, q0, steps, span=SPAN, flags=None, spans=None, region=True, lay=True):
        """anchors from (t0, q0) on by (dt, dq) steps; flags / spans: {chain index: value}.  -> (as, cnt)"""
        as_ = len(self.anchors)
        t, q = t0, q0
        pts = [(t, q)]
        for dt, dq in steps:
            t, q = t + dt, q + dq
            pts.append((t, q))
        for i, (t, q) in enumerate(pts):
            self.anchors.append(pb.anchor(rev, rid, t, q, (spans or {}).get(i, span), (flags or {}).get(i, 0)))
        if region:
            self.regions.append((0, as_, len(pts)))
        if lay:
            self.laid.append((rev, rid, pts))
        return as_, len(pts)

    def loose(self, rev, rid, pts, span=SPAN):
        """anchors of other chains, as they lie in the query's array: no region, nothing laid"""
        for t, q in pts:
            self.anchors.append(pb.anchor(rev, rid, t, q, span))

    def pin(self, kind, key, value):
        self.pins.setdefault(kind, {})[key] = value

    # -- sequences
    def _lay(self):
        for rev, rid, pts in self.laid:
            t = self.targets[rid]
            qa = revcomp(self.q) if rev else self.q.copy()
            for i, (tp, qp) in enumerate(pts):
                c = SPAN if i == 0 else min(tp - pts[i - 1][0], qp - pts[i - 1][1])
                c = min(c, tp + 1, qp + 1)
                qa[qp - c + 1:qp + 1] = t[tp - c + 1:tp + 1]
            self.q = revcomp(qa) if rev else qa

    def edit(self, rev, pos, code=None):
        """change the base at position pos of the aligned strand (after the chains were laid): the next base code, or the given one"""
        self.edits = getattr(self, "edits", []) + [(rev, pos, code)]

    def build(self):
        self._lay()
        for rev, pos, code in getattr(self, "edits", []):
            p = len(self.q) - 1 - pos if rev else pos
            if code is None:
                self.q[p] = (self.q[p] + 1) & 3
            else:
                self.q[p] = code if code > 3 or not rev else 3 - code
        seqs = ([_DUMMY] if self.base else []) + self.targets + [self.q]
        a = pb.anchors_array(self.anchors)
        tl = np.array([len(t) for t in self.targets])
        rid = ((a[:, 0] >> np.uint64(32)) & np.uint64(0x7fffffff)).astype(np.int64)
        assert (pb.tpos(a) >= HALF_K).all() and (pb.tpos(a) < tl[rid]).all() and (pb.qpos(a) + 1 >= (a[:, 1] >> np.uint64(32) & np.uint64(0xff)).astype(np.int64)).all() and (pb.qpos(a) < len(self.q)).all(), self.name
        return Group(self.name, seqs, self.base, [(len(seqs) - 1, a)], list(self.regions), dict(self.params), self.pins)


def diag(n, d=20):
    return [(d, d)] * n


def with_steps(n, at, d=20):
    """n diagonal steps of d with the steps of `at` = {chain index: (dt, dq)} put in (chain index i is the step that ends at anchor i)"""
    s = diag(n, d)
    for i, st in at.items():
        s[i - 1] = st
    return s


def indel_step(g, d=20):
    """a step whose query advance minus target advance is g"""
    return (d, d + g) if g > 0 else (d - g, d)


def _sizes(steps, t0=200, q0=200, room=400):
    return t0 + sum(s[0] for s in steps) + room, q0 + sum(s[1] for s in steps) + room


# ================================================================ extent and long-gap streaming
EXTENT_CNT = (1, 2, 3, 63, 64, 65, 66, 512, 513, 514, 1025)
_FIRST_LANES = (1, 65, 449, 513)                 # chain index 1; the first lane of the 2nd and of the 8th window; of the second trip
_INDELS = (10, -10, 11, -11, 30, -30, 31, -31)


def extent_cases():
    out = []
    for n, cnt in enumerate(EXTENT_CNT):
        for v in range(2):                       # two variants per length: which indel goes where, strand, short steps at the same places
            at, long_gaps = {}, 0
            for k, i in enumerate(p for p in _FIRST_LANES if p < cnt):
                g = _INDELS[(2 * n + 3 * k + 5 * v) % 8]
                at[i] = indel_step(g, 20 if (k + v) & 1 else 9)          # a step above the span on both sequences, or not
                long_gaps += abs(g) > 10
            for i in (2, 66, 450, 514):                                   # a short step (dt, dq <= span) right behind
                if i < cnt and v:
                    at[i] = (9, 9)
            steps = with_steps(cnt - 1, at)
            tl, ql = _sizes(steps)
            b = Builder(f"extent_cnt{cnt}_v{v}", [tl], ql, seed=100 + 2 * n + v, no_end_flt=1)
            b.chain(v, 0, 200, 200, steps)
            b.pin("out", (0, "n_long_gaps"), long_gaps)
            b.pin("out", (0, "as1"), 0)
            b.pin("out", (0, "cnt1"), cnt)
            b.pin("out", (0, "rev"), v)
            out.append(b.build())
    # a first anchor with tpos + 1 - span < 0: r_rs and rs0 are clamped at 0
    steps = diag(70)
    tl, ql = _sizes(steps, 10, 300)
    b = Builder("extent_tpos_below_span", [tl], ql, seed=150)
    b.chain(0, 0, 10, 300, steps)
    b.pin("out", (0, "r_rs"), 0)
    out.append(b.build())
    return out


# ================================================================ trimming (mm_fix_bad_ends)
def _trim(name, steps, pins, flags=None, back=False, **params):
    """back: the same walk from the other end (the steps reversed)"""
    if back:
        steps = steps[::-1]
        flags = {len(steps) - i + 1: f for i, f in (flags or {}).items()}      # blocks the same steps from the other side
    tl, ql = _sizes(steps)
    b = Builder(name + ("_back" if back else "_front"), [tl], ql, seed=len(name), **params)
    b.chain(0, 0, 200, 200, steps, flags=flags)
    cnt = len(steps) + 1
    for f, v in pins.items():
        if back:                                 # a front pin as1 = i becomes cnt1 = cnt - i
            assert f == "as1"
            b.pin("out", (0, "as1"), 0)
            b.pin("out", (0, "cnt1"), cnt - v)
        else:
            b.pin("out", (0, f), v)
            b.pin("out", (0, "cnt1"), cnt - v)
    return b.build()


def trim_cases():
    out = []
    for back in (False, True):
        far = dict(min_chain_score=100000, bw=100000)                       # no break condition within reach: only the off-diagonal test decides
        # hi - lo > len >> 1 with len = 15: 7 is not above, 8 is
        out.append(_trim("trim_offdiag7", with_steps(40, {1: (20, 27)}), {"as1": 0}, back=back, **far))
        out.append(_trim("trim_offdiag8", with_steps(40, {1: (20, 28)}), {"as1": 1}, back=back, **far))
        out.append(_trim("trim_no_end_flt", with_steps(40, {1: (20, 28)}), {"as1": 0}, back=back, no_end_flt=1, **far))
        # len >= bw << 1: steps of 17 from len 15; bw = 50: 100 after five steps (the walk ends before anchor 6), 99 with one step of 16
        lo = dict(min_chain_score=100000, bw=50)
        out.append(_trim("trim_len_eq", with_steps(200, {6: (17, 80)}, 17), {"as1": 0}, back=back, **lo))
        out.append(_trim("trim_len_below", with_steps(200, {3: (16, 16), 6: (17, 80)}, 17), {"as1": 6}, back=back, **lo))
        # match >= min_match and match >= bw: steps of 13 (below the span) from 15; min_match = 80: reached after five steps, 79 with one step of 12
        mm = dict(min_chain_score=40, bw=60)
        out.append(_trim("trim_match_eq", with_steps(200, {6: (13, 80)}, 13), {"as1": 0}, back=back, **mm))
        out.append(_trim("trim_match_below", with_steps(200, {3: (12, 12), 6: (13, 80)}, 13), {"as1": 6}, back=back, **mm))
        # match >= bw with min_match long reached: bw = 93 = 15 + 6 * 13 after six steps; 92 with one step of 12
        mb = dict(min_chain_score=10, bw=93)
        out.append(_trim("trim_match_bw_eq", with_steps(200, {7: (13, 80)}, 13), {"as1": 0}, back=back, **mb))
        out.append(_trim("trim_match_bw_below", with_steps(200, {3: (12, 12), 7: (13, 80)}, 13), {"as1": 7}, back=back, **mb))
        # match >= mlen >> 1: a chain of 12 anchors, steps of 13, one off-diagonal step (13, 50) adds 13: mlen = 15 + 11 * 13 = 158, half 79;
        # match is 80 after five steps; the off-diagonal step sits at anchor 6 (not seen) or at anchor 5 (seen: 50 - 13 > (15 + 4 * 13) >> 1)
        out.append(_trim("trim_mlen_after", with_steps(11, {6: (13, 50)}, 13), {"as1": 0}, back=back, **far))
        out.append(_trim("trim_mlen_before", with_steps(11, {5: (13, 50)}, 13), {"as1": 5}, back=back, **far))
        # an anchor flagged LONG_JOIN on input (a region split off earlier) stops the walk before the off-diagonal step behind it
        out.append(_trim("trim_long_join_stops", with_steps(40, {4: (20, 60)}), {"as1": 0}, flags={3: A_LONG_JOIN}, back=back, **far))
        out.append(_trim("trim_long_join_behind", with_steps(40, {4: (20, 60)}), {"as1": 4}, flags={5: A_LONG_JOIN}, back=back, **far))
    return out


# ================================================================ the cap on long gaps
def cap_cases():
    out = []
    for n_g, g_max in ((8, 8), (9, 8), (4096, 4096), (4097, 4096)):
        steps = [(12, 23)] * n_g + diag(3)                                    # every step an insertion of 11
        tl, ql = _sizes(steps)
        b = Builder(f"cap_{n_g}_of_{g_max}", [tl], ql, seed=n_g, g_max=g_max, no_end_flt=1)
        b.chain(0, 0, 200, 200, steps, lay=False)
        b.pin("out", (0, "status"), 2 if n_g > g_max else 0)
        if n_g <= g_max:
            b.pin("out", (0, "n_long_gaps"), n_g)
        out.append(b.build())
    return out


# ================================================================ indel bursts (mm_filter_bad_seeds)
def _filter_case(name, steps, ignore, join=(), **params):
    tl, ql = _sizes(steps)
    b = Builder(name, [tl], ql, seed=len(name) * 7, no_end_flt=1, **params)
    b.chain(0, 0, 200, 200, steps)
    b.pin("ignore", 0, set(ignore))
    b.pin("join", 0, set(join))
    return b.build()


def burst_cases():
    out = []
    I, D = indel_step, indel_step
    # weight 2 min(ins, del): 40 is not above the threshold, 42 is
    out.append(_filter_case("burst_w40", with_steps(30, {5: I(20), 8: D(-20)}), ()))
    out.append(_filter_case("burst_w42", with_steps(30, {5: I(21), 8: D(-21)}), range(5, 8)))
    # the partner is the 10th gap behind the first (reached) or the 11th (then the burst starts one gap later)
    at = {5: I(21)}
    at.update({6 + j: I(11) for j in range(9)})
    at[15] = D(-21)
    out.append(_filter_case("burst_partner_10th", with_steps(40, at), range(5, 15)))
    at = {5: I(21)}
    at.update({6 + j: I(11) for j in range(10)})
    at[16] = D(-21)
    out.append(_filter_case("burst_partner_11th", with_steps(40, at), range(6, 16)))
    # reach in bases, max_gap = 400: the partner's anchor is 200 (in) or 201 (out) behind the anchor in front of the first gap, on the query / on the target
    # anchor 4 -> 5 is the insertion of 25 (query + 45, target + 20); the deletion of 25 ends at anchor 7 (query + 20, target + 45)
    for axis in ("query", "target"):
        for over in (0, 1):
            if axis == "query":                  # query: 45 + 135 (+ over) + 20 = 200 (+ over); target: 20 + 134 + 45 = 199
                st = {5: I(25), 6: (134, 135 + over), 7: D(-25)}
            else:                                # target: 20 + 135 (+ over) + 45; query: 199
                st = {5: I(25), 6: (135 + over, 134), 7: D(-25)}
            # (the step at anchor 6 is itself off the diagonal by 1 or 2: not a long gap)
            out.append(_filter_case(f"burst_reach_{axis}_{'over' if over else 'eq'}", with_steps(30, st), () if over else range(5, 7), max_gap=400))
    # a stronger burst that starts inside an open one replaces it
    # (max_gap = 400.  From the deletion of 21 at anchor 5, the insertions of 11 at 7 and 8 give weight 42 and the deletion of 30 at anchor 10 is
    # out of reach, 251 target bases behind anchor 4; from the insertion at 7 it is 190 behind anchor 6 and gives 44)
    out.append(_filter_case("burst_replaced", with_steps(40, {5: (41, 20), 7: (20, 31), 8: (20, 31), 9: (100, 100), 10: (50, 20)}), range(7, 10), max_gap=400))
    # a burst that ends at the last long gap of the chain, which is the chain's last anchor
    out.append(_filter_case("burst_at_end", with_steps(20, {17: I(30), 20: D(-30)}), range(17, 20)))
    return out


# ================================================================ crowded gaps (mm_filter_bad_seeds_alt)
def crowded_cases():
    out = []
    I = indel_step
    # two insertions of 31 and 35 (no burst: same sign).  room = (tpos(j-1) + span) - t_end with j - 1 on the first gap's diagonal: 15 + the target
    # distance from the first gap's anchor (5) to anchor j - 1; g_prev + g = 66: distance 51 joins, 52 does not
    out.append(_filter_case("crowded_room_eq", with_steps(30, {5: I(31), 6: (17, 17), 7: (17, 17), 8: (17, 17), 9: I(35)}), range(5, 9), (9,)))
    out.append(_filter_case("crowded_room_over", with_steps(30, {5: I(31), 6: (17, 17), 7: (17, 17), 8: (18, 18), 9: I(35)}), ()))
    # reach, max_gap = 400: anchor j at most 200 behind the first gap's anchor on both sequences (room must still fit: gaps of 150)
    for over in (0, 1):
        st = {5: I(150), 6: (30, 30), 7: (20, 170 + over)}           # query: 30 + 170 (+ over) = 200 (+ over) behind anchor 5; an insertion of 150 (+ over)
        out.append(_filter_case(f"crowded_reach_query_{'over' if over else 'eq'}", with_steps(30, st), () if over else range(5, 7), () if over else (7,), max_gap=400))
        st = {5: I(-150), 6: (30, 30), 7: (170 + over, 20)}           # the same on the target, with deletions
        out.append(_filter_case(f"crowded_reach_target_{'over' if over else 'eq'}", with_steps(30, st), () if over else range(5, 7), () if over else (7,), max_gap=400))
    # three gaps joined in a row
    out.append(_filter_case("crowded_three", with_steps(40, {5: I(40), 7: I(45), 9: I(50)}), range(5, 9), (9,)))
    # exactly one gap above 30: nothing to join
    out.append(_filter_case("crowded_one_gap", with_steps(40, {5: I(40), 7: I(30), 9: I(12)}), ()))
    # gaps of 11 .. 30 between the gaps above 30 are skipped by the walk, and ignored with the rest
    out.append(_filter_case("crowded_small_between", with_steps(40, {5: I(40), 6: I(12), 7: I(30), 8: I(45)}), range(5, 8), (8,)))
    # both filters flag overlapping ranges: a burst (insertion 40, deletion 40) whose gaps are also crowded
    out.append(_filter_case("crowded_and_burst", with_steps(40, {5: I(40), 7: I(-40), 9: I(35)}), range(5, 9), (9,)))
    # an ignored range of 63, 64, 65 and 200 anchors: steps of one base between two insertions of 150
    for n in (63, 64, 65, 200):
        st = {5: I(150), 5 + n: I(150, 1)}
        st.update({5 + j: (1, 1) for j in range(1, n)})
        out.append(_filter_case(f"crowded_range_{n}", with_steps(n + 30, st), range(5, 5 + n), (5 + n,)))
    return out


# ================================================================ neighbour scans
def _scan_case(name, behind, pre=None, post=None, other_pre=None, other_post=None, chain_first=False, chain_last=False):
    """a diagonal chain of 30 anchors at (3000, 3000); pre / post: neighbour anchors on the same target and strand in array order, each
    'Q' (lies beyond the chain on both sequences; the k-th Q from the chain out is 100 k away), 't' / 'q' (beyond on that coordinate only);
    other_*: (position in the list, rev, rid) of an anchor of another target key put in.  The pin is the window end the deciding anchor gives."""
    steps = diag(29)
    b = Builder(name, [8000, 8000], 8000, seed=sum(map(ord, name)))
    t0 = q0 = 3000
    t_end, q_end = t0 + 20 * 29, q0 + 20 * 29

    def pts(lst, before):
        out, k = [], 0
        for c in lst:
            if c == "Q":
                k += 1
                d = 100 * k
                out.append((t0 + 1 - SPAN - d + SPAN - 1, q0 - d) if before else (t_end + d, q_end + d + 7 * k))
            elif c == "t":
                out.append((t0 - 500, q0 + 40) if before else (t_end + 500, q_end - 40))
            else:
                out.append((t0 + 40, q0 - 500) if before else (t_end - 40, q_end + 500))
        return out

    def put(lst, others, before):
        p = pts(lst, before)
        # array order: the scan walks away from the chain, so the backward list is stored reversed
        seq = [("n", x) for x in p]
        for at, rev, rid in (others or []):
            seq.insert(at, ("o", (rev, rid)))
        if before:
            seq = seq[::-1]
        for kind, x in seq:
            if kind == "n":
                b.loose(0, 0, [x])
            else:
                b.loose(x[0], x[1], [(4000, 4000)])

    if pre is not None and not chain_first:
        put(pre, other_pre, True)
    b.chain(0, 0, t0, q0, steps)
    if post is not None and not chain_last:
        put(post, other_post, False)
    return b


def scan_cases():
    out = []
    qs0_init = 3000 + 1 - SPAN
    qe0_init = 3000 + 20 * 29 + 1

    def add(name, lst, decider, others=None, **kw):
        """decider: which Q (1-based, counted from the chain) must decide, or None when the scan must find nothing"""
        for before in (True, False):
            b = _scan_case(f"scan_{name}_{'back' if before else 'fwd'}", before, pre=lst if before else None, post=None if before else lst,
                           other_pre=others if before else None, other_post=None if before else others, **kw)
            if before:
                # found: qs1 = qs0 - ll, ll = 100 k; not found: qs1 = max(0, qs - min(qs, max_gap)) = 0
                b.pin("out", (0, "qs0"), qs0_init - 100 * decider if decider else 0)
            else:
                b.pin("out", (0, "qe0"), qe0_init + 100 * decider + 7 * decider if decider else min(8000, qe0_init - 1 - HALF_K + 5000))
            out.append(b.build())

    add("first_window", ["Q"] * 6, 4)
    add("lane63", ["t"] * 60 + ["Q"] * 4 + ["Q"] * 3, 4)                       # the 4th qualifier is the 64th neighbour
    add("second_window", ["q"] * 61 + ["Q"] * 4 + ["Q"] * 3, 4)                 # ... the 65th
    add("split_2_2", ["t", "q"] * 31 + ["Q"] * 4 + ["Q"], 4)                    # qualifiers at neighbours 63, 64 | 65, 66
    add("one_coordinate_between", ["Q", "t", "Q", "q", "t", "Q", "q", "Q", "Q"], 4)
    add("second_window_late", ["Q"] + ["t"] * 70 + ["Q", "q", "Q", "Q", "Q"], 4)
    add("key_changes_inside", ["Q", "Q", "Q", "Q", "Q"], None, others=[(3, 0, 1)])      # another target after three qualifiers
    add("key_changes_at_edge", ["Q", "Q", "Q"] + ["t"] * 61 + ["Q", "Q"], None, others=[(64, 0, 1)])   # ... exactly at neighbour 65
    add("key_changes_after_edge", ["Q", "Q", "Q"] + ["t"] * 61 + ["Q", "Q"], 4, others=[(65, 0, 1)])
    add("other_strand_neighbour", ["Q", "Q", "Q", "Q", "Q"], None, others=[(2, 1, 0)])  # the same target on the other strand ends the walk
    add("too_few", ["Q", "t", "Q", "q", "Q"], None)
    add("none", [], None)
    # as = 0 / the chain ends at the array's end: no neighbour on that side
    b = _scan_case("scan_as0", True, pre=None, post=["Q"] * 5)
    b.pin("out", (0, "qs0"), 0)
    out.append(b.build())
    b = _scan_case("scan_chain_at_array_end", False, pre=["Q"] * 5, post=None)
    b.pin("out", (0, "qe0"), min(8000, qe0_init - 1 - HALF_K + 5000))
    out.append(b.build())
    return out


# ================================================================ windows
def window_cases():
    out = []

    def case(name, t0, q0, tlen=None, qlen=None, first_span=8, pins=(), flags=None, steps=None, **params):
        steps = steps or diag(20)
        tl, ql = _sizes(steps, t0, q0)
        b = Builder(name, [tlen or tl], qlen or ql, seed=len(name) * 3, **params)
        b.chain(0, 0, t0, q0, steps, spans={0: first_span}, flags=flags)
        for f, v in pins:
            b.pin("out", (0, f), v)
        out.append(b.build())

    far = dict(min_chain_score=100000, bw=100000)
    # qs = 0 / rs = 0: no left extension, the windows start at the chain (first span 8, so that qpos + 1 - span >= 0 at qpos = k/2)
    case("win_qs0", 500, 7, pins=(("qs", 0), ("qs0", 0), ("rs0", 493)), **far)
    case("win_rs0", 7, 500, pins=(("rs", 0), ("rs0", 0), ("qs0", 493)), **far)
    # l a against q with a = 2, q = 4, e = 2 and a first span of 8 (rs0 starts at rs): l = qs = 2 is equal (rs0 = rs - 2), l = 3 is above (l becomes 4)
    case("win_la_eq", 500, 9, pins=(("qs", 2), ("qs0", 0), ("rs0", 491)), **far)
    case("win_la_above", 500, 10, pins=(("qs", 3), ("qs0", 0), ("rs0", 489)), **far)
    # max_gap clamps l on the query (qs0 = qs - max_gap), and again after the gap-cost extension
    case("win_max_gap", 1000, 1000, pins=(("qs0", 993 - 100), ("rs0", 993 - 100)), max_gap=100, **far)
    # rs clamps l on the target
    case("win_rs_clamp", 50, 1000, pins=(("rs0", 0), ("qs0", 0)), **far)
    # the right side: tlen - re clamps; max_gap clamps
    steps = diag(20)
    t_last, q_last = 500 + 400, 500 + 400
    case("win_tlen_clamp", 500, 500, tlen=t_last + 30, qlen=q_last + 1000, pins=(("re0", t_last + 30), ("qe0", q_last + 1000)), **far)
    case("win_right_max_gap", 500, 500, tlen=t_last + 1000, qlen=q_last + 1000, pins=(("qe0", q_last - 7 + 100), ("re0", t_last - 7 + 100)), max_gap=100, **far)
    # an A_SELF chain 30 off the main diagonal: max_ext = 30 on either side clamps all four ends
    case("win_self", 1000, 1030, first_span=15, flags={0: A_SELF}, tlen=3000, qlen=3000,
         pins=(("rs0", 1000 + 1 - 15 - 30), ("qs0", 1030 + 1 - 15 - 30), ("re0", 1401 + 30), ("qe0", 1431 + 30)), **far)
    return out


# ================================================================ the cut
def cut_cases():
    out = []

    def case(name, steps, segs, flags=None, join=None, **params):
        tl, ql = _sizes(steps)
        b = Builder(name, [tl], ql, seed=len(name) * 5, **{**dict(min_ksw_len=40, no_end_flt=1), **params})
        b.chain(0, 0, 200, 200, steps, flags=flags)
        b.pin("segs", 0, segs)
        if join is not None:
            b.pin("join", 0, set(join))
        out.append(b.build())

    # steps of 20: a cut at every second anchor, 32 in a window
    case("cut_many_per_window", diag(200), 100)
    # three cuts inside one window, none elsewhere: steps of one base (200 in all, below min_ksw_len = 300), three steps of 300 in the second window,
    # and the closing segment
    B = (300, 300)
    case("cut_three_in_window", with_steps(200, {70: B, 90: B, 110: B}, 1), 4, min_ksw_len=300)
    # a cut at lane 0 (chain index 1, 65) and at lane 63 (chain index 64, 128)
    case("cut_lane0", with_steps(200, {1: B, 65: B}, 1), 3, min_ksw_len=300)
    case("cut_lane63", with_steps(200, {64: B, 128: B}, 1), 3, min_ksw_len=300)
    # a segment spanning three windows without a cut
    case("cut_span_three_windows", diag(200, 1), 1, min_ksw_len=300)
    # a window whose anchors are all flagged: 65 .. 128 TANDEM, then IGNORE; steps of 20
    # (cuts at 2, 4 .. 64, then at the first anchor behind the flagged window, 129, at 131 .. 199, and the closing segment at 200)
    case("cut_window_tandem", diag(200), 32 + 36 + 1, flags={i: A_TANDEM for i in range(65, 129)})
    case("cut_window_ignore", diag(200), 32 + 36 + 1, flags={i: A_IGNORE for i in range(65, 129)})
    # a flagged last anchor still closes
    case("cut_last_flagged", diag(11), 4 + 1, flags={11: A_TANDEM, 10: A_TANDEM})
    # a LONG_JOIN anchor cuts whatever the lengths, with bw1 = the longer window (on input, and set by the crowded-gap filter)
    case("cut_long_join_input", with_steps(30, {5: (3, 90)}), 15 + 1, flags={5: A_LONG_JOIN})
    case("cut_long_join_filter", with_steps(40, {5: indel_step(40), 7: indel_step(45)}), None, join=(7,))
    # the query long enough but the target not, and the other way round: no cut until both are
    # (indels of 10, not long gaps: the query reaches 40 at anchor 2, the target at anchor 4)
    case("cut_query_only", with_steps(6, {1: (10, 20), 2: (10, 20), 3: (10, 20)}), 2)
    case("cut_target_only", with_steps(6, {1: (20, 10), 2: (20, 10), 3: (20, 10)}), 2)
    for cnt1 in (1, 2, 64, 65, 66, 129):
        case(f"cut_cnt{cnt1}", diag(cnt1 - 1), cnt1 // 2)
    return [g for g in out]


# ================================================================ probes
def probe_cases():
    """two-anchor chains on the main diagonal: one segment of exactly L bases, [t0 - 7, t0 - 7 + L) against the same stretch of the aligned query"""
    out = []

    def case(name, L, edits, item, rev=0, q0=300, seq_edit=None, **params):
        b = Builder(name, [1500], 1500, seed=len(name) * 11 + L, min_ksw_len=1, no_end_flt=1, **params)
        # the aligned strand copies the target around the chain
        t = b.targets[0]
        qa = t.copy()[:1500]
        b.q = revcomp(qa) if rev else qa
        b.chain(rev, 0, q0, q0, [(L, L)], lay=False)
        for e in edits:
            b.edit(rev, q0 - HALF_K + e[0], e[1] if len(e) > 1 else None)
        if seq_edit:
            t[q0 - HALF_K + seq_edit[0]] = seq_edit[1]
            # (the query was copied before: the target alone carries the code)
        b.pin("items", 0, [item])
        out.append(b.build())

    big = 30001                                   # bw_long * 1.5 + 1
    for L in (1, 63, 64, 65, 129):
        case(f"probe_len{L}_clean", L, [], (0, 1, 0))
        case(f"probe_len{L}_m_max", L, [(j,) for j in sorted({0, L - 1})], (0, 1, len({0, L - 1})))
        n = 3
        pos = sorted({0, L - 1, L // 2, L // 3})[:n]
        if len(pos) == 3:
            case(f"probe_len{L}_m_over", L, [(j,) for j in pos], (2, big, 0))
    # the deciding (third) mismatch in the first base, the last base, lane 0 of the second trip
    case("probe_decides_first", 129, [(0,), (50,), (100,)], (2, big, 0))
    case("probe_decides_last", 129, [(128,), (50,), (100,)], (2, big, 0))
    case("probe_decides_lane0_trip2", 129, [(64,), (10,), (20,)], (2, big, 0))
    case("probe_two_at_trip_edge", 129, [(63,), (64,)], (0, 1, 2))
    # an N as the last base of either window
    case("probe_n_last_query", 65, [(64, 4)], (2, big, 0))
    case("probe_n_last_target", 65, [], (2, big, 0), seq_edit=(64, 4))
    case("probe_n_behind_query", 65, [(65, 4)], (0, 1, 0))
    # probe_m_max -1 (no probe at all) and 0
    case("probe_off", 64, [], (2, big, 0), probe_m_max=-1)
    case("probe_m0_clean", 64, [], (0, 1, 0), probe_m_max=0)
    case("probe_m0_one", 64, [(33,)], (2, big, 0), probe_m_max=0)
    # ql tl at max_sw_mat and one above
    case("probe_sw_mat_eq", 64, [], (0, 1, 0), max_sw_mat=4096)
    case("probe_sw_mat_over", 64, [], (2, big, 0), max_sw_mat=4095)
    # a reverse-strand query whose window starts at every residue modulo the sixteen bases of a packed word (forward position of the window's
    # first base: qlen - 1 - qs), clean and with a mismatch in the first and last base
    for r in range(16):
        case(f"probe_rev_res{r}_clean", 65, [], (0, 1, 0), rev=1, q0=300 + r)
        case(f"probe_rev_res{r}_ends", 65, [(0,), (64,)], (0, 1, 2), rev=1, q0=300 + r)
        case(f"probe_rev_res{r}_over", 65, [(0,), (1,), (64,)], (2, big, 0), rev=1, q0=300 + r)
    return out


# ================================================================ collapse
def collapse_cases():
    """n segments of 40 bases on the main diagonal; `hard` segments carry three mismatches, `one` segments one"""
    out = []

    def case(name, n, hard=(), one=(), items=None):
        L = 40
        size = 300 + L * n + 300
        b = Builder(name, [size], size, seed=n * 13 + len(name), min_ksw_len=L, no_end_flt=1)
        b.q = b.targets[0].copy()
        b.chain(0, 0, 300, 300, [(L, L)] * n, lay=False)
        for s in hard:
            for j in (3, 17, 31):
                b.edit(0, 300 - HALF_K + L * s + j)
        for s in one:
            b.edit(0, 300 - HALF_K + L * s + 11)
        b.pin("segs", 0, n)
        b.pin("items", 0, items)
        out.append(b.build())

    big = 30001
    H = (2, big, 0)
    for n in (64, 65, 128, 129):
        case(f"collapse_{n}_all_answered", n, items=[(0, n, 0)])
        case(f"collapse_{n}_none", n, hard=range(n), items=[H] * n)
        case(f"collapse_{n}_alternating", n, hard=range(0, n, 2), items=[x for s in range(n) for x in ([H] if s % 2 == 0 else [(0, 1, 0)])])
    for s in (0, 63, 64):
        case(f"collapse_hard_slot{s}", 130, hard=(s,), items=([(0, s, 0)] if s else []) + [H, (0, 129 - s, 0)])
    # a run open across two window edges; its mismatches sum across them: segments 60 .. 135 answered, one mismatch in 62, 63, 64, 100, 127, 128, 135
    one = (62, 63, 64, 100, 127, 128, 135)
    case("collapse_run_across_edges", 140, hard=(59, 136), one=one, items=[(0, 59, 0), H, (0, 76, len(one)), H, (0, 3, 0)])
    return out


# ================================================================ the host sequence
def _many_regions(name, n_regions, anchors_per, step, **params):
    size = 300 + n_regions * (anchors_per * step + 5) + 300
    b = Builder(name, [size], size, seed=n_regions, **params)
    for r in range(n_regions):
        p = 300 + r * (anchors_per * step + 5)
        b.chain(0, 0, p, p, [(step, step)] * (anchors_per - 1), lay=False)
    return b


def host_cases():
    out = []
    # 1025 regions of one anchor pair: above the zero-copy limit of 1024, everything goes through device copies
    b = _many_regions("host_1025_regions", 1025, 2, 30, no_end_flt=1)
    b.pin("segs", 1024, 1)
    out.append(b.build())
    # 1024 regions with nine hard segments each: 9216 items, above eight per region: records through pinned memory, items through a device copy
    b = _many_regions("host_1024_regions_9216_items", 1024, 10, 40, min_ksw_len=40, no_end_flt=1)
    b.pin("segs", 1023, 9)
    b.pin("items", 1023, [(2, 30001, 0)] * 9)
    out.append(b.build())
    # an empty chain (status 3) and a chain over the cap (status 2) between normal ones: their item offsets are skipped
    steps = [(12, 23)] * 9 + diag(3)
    b = Builder("host_status_mix", [3000], 3000, seed=77, g_max=8, min_ksw_len=40, no_end_flt=1)
    b.chain(0, 0, 200, 200, diag(10))
    b.regions.append((0, 3, 0))
    b.chain(0, 0, 600, 600, steps, lay=False)
    b.chain(0, 0, 1200, 1200, diag(10))
    for r, st in enumerate((0, 3, 2, 0)):
        b.pin("out", (r, "status"), st)
    out.append(b.build())
    b = Builder("host_empty_list", [500], 500, seed=3)
    b.loose(0, 0, [(100, 100), (120, 120)])
    out.append(b.build())
    return out


# ================================================================ random groups
N_RANDOM = 40


def random_group(seed):
    """two targets, one query built from them: 3 - 6 chains in disjoint slots of the forward query, on either target and strand, indels drawn around
    10 and 30, a few percent of substitutions afterwards"""
    rng = np.random.default_rng(9000 + seed)
    n_chains = int(rng.integers(3, 7))
    W = 2600
    qlen = W * n_chains + 200
    b = Builder(f"random_{seed}", [W * 3, W * 3], qlen, seed=9000 + seed, min_ksw_len=int(rng.choice([60, 200])), base=int(seed % 4 != 0))
    specs = []
    for c in range(n_chains):
        rev, rid = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        n = int(rng.integers(5, 90))
        steps = []
        for _ in range(n):
            d = int(rng.integers(8, 30))
            if rng.random() < 0.12:
                g = int(rng.choice([10, 30])) + int(rng.integers(-2, 4))
                steps.append(indel_step(g if rng.random() < 0.5 else -g, d))
            else:
                steps.append((d, d))
        dq, dt = sum(s[1] for s in steps), sum(s[0] for s in steps)
        while dq > W - 200 or dt > W - 200:
            steps.pop()
            dq, dt = sum(s[1] for s in steps), sum(s[0] for s in steps)
        lo = c * W + 100                                                  # the slot on the forward strand
        q0 = (qlen - (lo + W - 200)) if rev else lo
        q0 = max(q0, 20) + int(rng.integers(0, 60))
        specs.append((rev, rid, int(rng.integers(50, 2 * W)), q0, steps))
    for rev, rid, t0, q0, steps in sorted(specs, key=lambda s: (s[0], s[1], s[2])):     # same target and strand side by side, as the chain stage leaves them
        b.chain(rev, rid, t0, q0, steps)
    g = b.build()
    sub = np.nonzero(rng.random(qlen) < 0.02)[0]
    q = g.seqs[-1]
    q[sub] = (q[sub] + 1 + rng.integers(0, 3, len(sub))) & 3
    return g


def random_groups():
    return [random_group(s) for s in range(N_RANDOM)]


FAMILIES = dict(extent=extent_cases, trim=trim_cases, cap=cap_cases, burst=burst_cases, crowded=crowded_cases, scan=scan_cases, window=window_cases,
                cut=cut_cases, probe=probe_cases, collapse=collapse_cases, host=host_cases, random=random_groups)
_CACHE = {}


def family(name):
    """the groups of a family, built once per process (treat as read-only)"""
    if name not in _CACHE:
        _CACHE[name] = FAMILIES[name]()
        names = [g.name for g in _CACHE[name]]
        assert len(set(names)) == len(names), names
    return _CACHE[name]
