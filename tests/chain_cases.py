"""Anchor-level cases for the chain sweep (pangraph_amd/csrc/pga_chain.hip), built on purpose and not from sequences.

The edges of the sweep depend on exact anchor geometry: 64-anchor block edges, the ring capacity 2 048, the inner window 256 / 1 024, equal
priorities, equal x, WGS_CAP.  Every case is a list of queries, each query a (n, 2) uint64 array of anchors (x, y) in the order mg_lchain_rmq
would receive them (ascending x; anchors sharing x by ascending y), plus its parameter set.  Pure numpy, deterministic seeds, no GPU.

  x = strand << 63 | target << 32 | target position        y = span << 32 | query position        (minimap.h: mm128_t anchors)

tests/test_chain_cases_cpu.py pins, on the CPU, the properties the GPU assertions rely on (a vacuous case fails there); the counters a case
is meant to raise on the device are asserted in tests/test_gpu_chain_routes.py.
"""
from dataclasses import dataclass, field, replace

import numpy as np

SPAN = 19


@dataclass(frozen=True)
class Params:
    """the chaining parameters of mg_lchain_rmq; the default is asm10's (make_options("asm10"))"""
    max_gap: int = 10_000
    rmq_inner_dist: int = 1_000
    bw: int = 1_000
    max_chain_skip: int = 25
    rmq_size_cap: int = 100_000
    min_cnt: int = 3
    min_chain_score: int = 40
    chain_gap_scale: float = 0.8
    chain_skip_scale: float = 0.0
    k: int = 19


ASM10 = Params()


@dataclass
class Case:
    name: str
    group: str
    queries: list                      # of (n, 2) uint64 arrays
    params: Params = ASM10
    chains: bool = True                # the case is meant to yield at least one chain
    pins: dict = field(default_factory=dict)   # properties test_chain_cases_cpu.py checks (see there)


def mk(pos, qpos, rid=0, strand=0, span=SPAN):
    """anchors from arrays (or scalars) of target position, query position, target, strand, span -> (n, 2) uint64, sorted by (x, y)"""
    pos, qpos, rid, strand, span = np.broadcast_arrays(np.atleast_1d(pos), np.atleast_1d(qpos), rid, strand, span)
    x = (strand.astype(np.uint64) << np.uint64(63)) | (rid.astype(np.uint64) << np.uint64(32)) | pos.astype(np.uint64)
    y = (span.astype(np.uint64) << np.uint64(32)) | qpos.astype(np.uint64)
    a = np.stack([x, y], axis=1)
    return np.ascontiguousarray(a[np.lexsort((a[:, 1], a[:, 0]))])


def cat(*parts):
    a = np.concatenate([p for p in parts if len(p)], axis=0) if any(len(p) for p in parts) else np.zeros((0, 2), np.uint64)
    return np.ascontiguousarray(a[np.lexsort((a[:, 1], a[:, 0]))])


EMPTY = np.zeros((0, 2), np.uint64)


def diag(n, x0=1000, y0=500, step=10, **kw):
    i = np.arange(n, dtype=np.int64)
    return mk(x0 + step * i, y0 + step * i, **kw)


def diag_steps(steps, x0=1000, y0=500, **kw):
    d = np.concatenate([[0], np.cumsum(np.asarray(steps, dtype=np.int64))])
    return mk(x0 + d, y0 + d, **kw)


# ------------------------------------------------------------------------------------------------ co-linear stretch
COLINEAR_LENGTHS = (1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200)


def _colinear_queries():
    out = {}
    out["step10"] = [diag(n, step=10) for n in COLINEAR_LENGTHS]                       # dr == dq <= span: "exact", the stretch
    out["step30"] = [diag(n, step=30) for n in COLINEAR_LENGTHS]                       # dd == 0 but dg > span: single shortcut + bound / inner scan
    # the step alternates so that stretches of 1, 2 and 3 anchors occur (R >= 2 boundary): 30 breaks a stretch, 10 continues one
    pat = [30, 10, 30, 10, 10, 30, 10, 10, 10, 30, 30]
    out["alternating"] = [diag_steps((pat * 20)[:n]) for n in (11, 66, 131, 200)]
    # a stretch broken by one anchor whose own span is not below what the stretch would give it (f_l <= span): it starts a chain of its own
    q = []
    for at in (5, 62, 63, 64, 70):
        n = 140
        i = np.arange(n, dtype=np.int64)
        span = np.full(n, SPAN, dtype=np.int64)
        span[at] = 255                                                                   # f of the stretch at slot 5 is 69, at slot 70 it is 719 > 255
        q.append(mk(1000 + 10 * i, 500 + 10 * i, span=span))
    out["broken"] = q
    return out


def colinear_cases(params=ASM10, group="colinear", suffix=""):
    return [Case(f"colinear_{k}{suffix}", group, v, params) for k, v in _colinear_queries().items()]


# ------------------------------------------------------------------------------------------------ the f + span bound
def bound_case():
    """The bound that skips the inner scan must count the anchor just below i when the range minimum is somebody else.  A diagonal of 100 anchors
    ends in j (f = 1009); anchor i - 1 has span 200, sits 35 off the diagonal below j (f = 972: lower priority than j); i follows 150 on, on j's
    diagonal.  The range minimum is j (dd == 0: 1009 + 19, exactly what f + span of every anchor up to j allows), but i - 1 gives 972 + 145 - 7"""
    q = cat(diag(100, x0=1000, y0=1000), mk([1995], [1960], span=200), mk([2140], [2140]))
    return Case("bound_last_anchor", "shortcut_edges", [q], pins=dict(last_p=100, last_f=1110))


def y_range_edge_case():
    """The single shortcut takes the anchor just below only if it lies inside the y range of the range-min query, (y_i - max_dist, y_i).  A diagonal
    of 200 anchors (f = 2009), then an anchor 10 on in x and exactly max_dist on in y: its neighbour is outside, nobody else is inside, it stays
    unchained.  With max_dist - 1 the neighbour is inside and, bw being max_dist here, within the band: chained at a cost of ~1 520"""
    p = replace(ASM10, bw=10_000)
    return Case("y_range_edge", "shortcut_edges", [cat(diag(200), mk([1000 + 2000], [500 + 1990 + dy])) for dy in (10_000, 9_999)], p, pins=dict(last_ps=[-1, 199]))


def inner_y_edge_case():
    """The inner scan takes candidates with y in [y_i - rmq_inner_dist, y_i - 1], both ends included.  Anchor i = (3000, 5000); the range minimum is an
    anchor of span 255 far off the diagonal (outside the band: nothing chained, not "exact", so the inner scan runs); the only anchor i can chain to
    lies 990 back in x and exactly rmq_inner_dist back in y -- found by the inner scan alone.  One further back in y it is outside: i stays unchained"""
    return Case("inner_y_edge", "shortcut_edges", [cat(mk([2010], [5000 - dy]), mk([2995], [2500], span=255), diag(10, x0=3000, y0=5000)) for dy in (1000, 1001)],
                pins=dict(p_at={(0, 2): 0, (1, 2): -1}, f_at={(0, 1): 255, (1, 2): SPAN}))


def evicted_minimum_case():
    """A block summary may stand in for a partly evicted block only while the block's minimum is still in the window.  Block 0: a head of span 255 at
    x = 100 (the block's unique minimum) and 63 anchors that chain to nobody (x ascends from 300, y descends).  Anchor 64 at x = 10 150 sees the block
    wholly inside its y range, the head evicted (10 050 away), the others not: none of them is within the band, it stays unchained -- the head would
    have been (dd = 150)"""
    t = np.arange(63, dtype=np.int64)
    q = cat(mk([100], [100], span=255), mk(300 + t, 2000 - 10 * t), diag(10, x0=10_150, y0=10_000))
    return Case("evicted_minimum", "summary", [q], pins=dict(p_at={(0, 64): -1}, f_at={(0, 64): SPAN, (0, 0): 255}))




# ------------------------------------------------------------------------------------------------ ring overflow, tree-size cap
def dense_diagonal(s, n=2600, seed=11):
    """x = 100 + s i, y = x +- 1: about max_gap / s anchors in the live window"""
    rng = np.random.default_rng(seed + s)
    x = 100 + s * np.arange(n, dtype=np.int64)
    return mk(x, x + rng.choice(np.array([-1, 1]), size=n))


def overflow_cases():
    return [Case("overflow_s4", "overflow_s4", [dense_diagonal(4)], pins=dict(window_min=2049)),       # blk + 128 - st > 2048 must happen
            Case("overflow_s6", "overflow_s6", [dense_diagonal(6)], pins=dict(window_max=2048 - 128))]  # ... and must not


def cap_cases():
    out = []
    for cap in (50, 1000):
        p = replace(ASM10, rmq_size_cap=cap)
        for s in (4, 6):
            out.append(Case(f"cap{cap}_s{s}", "cap", [dense_diagonal(s)], p, pins=dict(window_min=cap + 1)))
    p = replace(ASM10, rmq_size_cap=1000)
    # below 2 048 the shortcut is switched off: every anchor of an otherwise co-linear case takes the scan and summary path
    out += colinear_cases(p, "cap", "_cap1000")
    out += [replace(c, name=c.name + "_cap1000", group="cap", params=p) for c in summary_cases()]
    return out


# ------------------------------------------------------------------------------------------------ tied minimum
def _fillers(n):
    """n anchors that neither chain to one another nor to anything above them: x ascends, y descends"""
    t = np.arange(n, dtype=np.int64)
    return mk(100 + t, 2000 - 10 * t)


def tie_cases():
    tail = diag(30, x0=3300, y0=3300)
    # (a) two chain heads with equal f (their span) and equal x + y in one 64-block, both inside the y range of a later diagonal
    a = cat(mk([100, 200], [200, 100]), diag(30, x0=300, y0=300))
    # (b) heads in different blocks: block 0 ends with two heads of equal priority, so its summary has no unique minimum (sm_arg < 0); the
    #     third head opens block 1; the fillers' priorities lie above (x + y smaller, same f)
    b = cat(_fillers(62), mk([2900, 3000, 3100], [300, 200, 100]), tail)
    # (c) the tie inside a partly evicted block: by the time the diagonal is reached the fillers have left the window, the heads have not
    c = cat(_fillers(62), mk([9000, 9100], [300, 200]), diag(30, x0=10300, y0=3300))
    return [Case("tie_same_block", "tie", [a], pins=dict(tie=True)),
            Case("tie_summary", "tie", [b], pins=dict(tie=True, n_first_block=64)),
            Case("tie_partly_evicted", "tie", [c], pins=dict(tie=True))]


# ------------------------------------------------------------------------------------------------ block summaries
def scatter(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 60_000, size=n)
    y = x + 3000 + rng.integers(-3000, 3001, size=n)
    a = np.unique(np.stack([x, y], axis=1), axis=0)
    return mk(a[:, 0], a[:, 1])


def two_diagonals(n=1500, seed=6):
    """two parallel diagonals 300 apart, a path that hops between them at random, and strays on the other one"""
    rng = np.random.default_rng(seed)
    x = 1000 + 12 * np.arange(n, dtype=np.int64)
    on = np.cumsum(rng.random(n) < 0.05) & 1
    stray = rng.random(n) < 0.3
    return cat(mk(x, x + 300 * on), mk(x[stray], x[stray] + 300 * (1 - on[stray])))


def summary_cases():
    return [Case("scatter", "summary", [scatter()]), Case("two_diagonals", "summary", [two_diagonals()])]   # (+ evicted_minimum_case: all_cases)


# ------------------------------------------------------------------------------------------------ crowded and unsorted inner windows
def grid(n, seed=9):
    """jittered n x n grid: the jitter breaks priority ties, which would otherwise pre-empt the inner scan with a tied minimum"""
    rng = np.random.default_rng(seed + n)
    i, j = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    x = 1000 + 25 * i.ravel() + rng.integers(0, 8, size=n * n)
    y = 1000 + 25 * j.ravel() + rng.integers(0, 8, size=n * n)
    a = np.unique(np.stack([x, y], axis=1), axis=0)
    return mk(a[:, 0], a[:, 1])


def grid_rc(cols, rows, seed):
    """jittered grid of cols columns (x) by rows rows (y), 25 apart"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(cols, dtype=np.int64), np.arange(rows, dtype=np.int64), indexing="ij")
    x = 1000 + 25 * i.ravel() + rng.integers(0, 8, size=cols * rows)
    y = 1000 + 25 * j.ravel() + rng.integers(0, 8, size=cols * rows)
    a = np.unique(np.stack([x, y], axis=1), axis=0)
    return mk(a[:, 0], a[:, 1])


WRAP_SEEDS = {(60, 20): 1, (200, 6): 0}     # (seeds without a tied minimum: pinned by the CPU test)


def wrap_cases():
    """segments of more than 1 024 anchors whose inner windows stay below the hand-over: the predecessor and stamp rings of the inner scan (1 024
    slots) wrap, and a chain head's missing predecessor (-1) must not stamp slot 1 023.  40 columns lie inside rmq_inner_dist: 20 rows fill the
    chunked form (about 800 candidates), 6 rows the register form (about 240)"""
    out = []
    for (cols, rows), seed in WRAP_SEEDS.items():
        lo, hi = (257, 1024) if rows == 20 else (65, 256)
        for skip in (0, 2):
            out.append(Case(f"wrap{cols}x{rows}_skip{skip}", "wrap", [grid_rc(cols, rows, seed)], replace(ASM10, max_chain_skip=skip),
                            pins=dict(inner_min=lo, inner_max=hi, no_tie=True, n_min=1025)))
    return out


def grid_cases():
    out = []
    # anchors inside rmq_inner_dist of one anchor: at most CF_MAXIN = 256 (the register form), at most CF_WI = 1 024 (the chunked form), more (hand-over)
    for n, lo, hi in ((12, 65, 256), (20, 257, 1024), (34, 1025, None)):
        for skip in (0, 2, 25):
            out.append(Case(f"grid{n}_skip{skip}", f"grid{n}", [grid(n)], replace(ASM10, max_chain_skip=skip), pins=dict(inner_min=lo, inner_max=hi, no_tie=True)))
    return out


# ------------------------------------------------------------------------------------------------ equal x
def equal_x_case():
    """runs of 2-5 anchors sharing x (late insertion, i0): one at the very start of the segment, runs that straddle slots 62..66 and 126..130"""
    runs = {0: 3, 20: 2, 62: 5, 100: 4, 126: 5, 150: 2}
    pos, qpos, slot, t = [], [], 0, 0
    while slot < 200:
        r = runs.get(slot, 1)
        for k in range(r):
            pos.append(1000 + 10 * t); qpos.append(500 + 10 * t + 7 * k)
        slot += r; t += 1
    q = mk(pos, qpos)
    starts = [s for s in runs]
    return Case("equal_x", "equal_x", [q], pins=dict(equal_x_runs=starts))


# ------------------------------------------------------------------------------------------------ segmentation
def segmentation_cases():
    d = diag(30)
    batch = [EMPTY, EMPTY, d, EMPTY, diag(1), diag(2), diag(30, x0=5000, y0=100), EMPTY, EMPTY]
    strands = cat(*[diag(10 + 3 * r + s, x0=1000 + 100 * r, y0=500 + 1000 * (3 * s + r), rid=r, strand=s) for s in (0, 1) for r in (0, 1, 2)])
    out = [Case("seg_batch", "segmentation", batch), Case("seg_strands_targets", "segmentation", [strands])]

    def jump(gap):                                   # the second diagonal joins the first one's chain unless a segment cut lies between them
        a = diag(12)
        xe, ye = 1000 + 110, 500 + 110
        return cat(a, diag(12, x0=xe + gap, y0=ye + gap - 10))
    out.append(Case("seg_jump_max_gap", "segmentation", [jump(10_000), jump(10_001)], pins=dict(n_chains=[1, 2])))
    wide = replace(ASM10, bw=12_000)
    out.append(Case("seg_jump_bw", "segmentation", [jump(12_000), jump(12_001)], wide, pins=dict(n_chains=[1, 2])))
    # the (y_i, 0) upper key (lchain.c:310) is in QUERY numbering: an anchor with y == y_i is inside the range-min query only as anchor 0 of the whole
    # query.  It can never be chained to (dq == 0), but where it is the range minimum it keeps the query from finding anybody else: here an anchor b
    # that lies outside the inner window, so that the inner scan does not find it either.  The third anchor stays unchained at query index 0 and chains
    # to b (f = 20) behind a segment cut, where the same head is anchor 0 of the segment only
    def triple(x0):
        return mk([x0, x0 + 50, x0 + 1250], [5000, 3900, 5000])
    q0 = cat(triple(100), diag(8, x0=2100, y0=6000), triple(30_000), diag(8, x0=32_000, y0=6000))
    q1 = cat(triple(100), diag(8, x0=2100, y0=6000))
    out.append(Case("seg_y_equal_index0", "segmentation", [q0, q1], pins=dict(index0=True)))
    return out


# ------------------------------------------------------------------------------------------------ small-sort edges (WGS_CAP = 4096)
def sort_edge_cases():
    out = []
    for n_q in (4096, 4097):                         # the segment sort: one segment per query, lengths 3..6
        out.append(Case(f"segments_{n_q}", "sort_edges", [diag(3 + q % 4, x0=1000 + q, y0=500 + 2 * q, step=15) for q in range(n_q)]))
    for n_a in (4096, 4097):                         # the candidate sort
        lens = [256] * 15 + [n_a - 256 * 15]
        out.append(Case(f"anchors_{n_a}", "sort_edges", [diag(n, x0=1000 + 3 * q, y0=500 + q) for q, n in enumerate(lens)], pins=dict(n_anchors=n_a)))
    return out


# ------------------------------------------------------------------------------------------------ backtrack
def interleaved(n_diag, base_len=20):
    """n_diag diagonals 20 000 apart in y, interleaved in x: every predecessor lies n_diag slots below.  Diagonal d is base_len + d anchors long, so
    that no two chains score alike"""
    pos, qpos = [], []
    for s in range(base_len + n_diag):
        for d in range(n_diag):
            if s < base_len + d:
                pos.append(1000 + 700 * s + 10 * d); qpos.append(500 + 20_000 * d + 700 * s)
    return mk(pos, qpos)


def max_drop_chain():
    """a long diagonal, ten hops of 900 off the diagonal (each costs ~120: more than max_drop = bw in all), a long diagonal: the walk back from the
    end is cut inside the hops, the first diagonal chains on its own"""
    a = diag(300)
    x, y = 1000 + 2990, 500 + 2990
    hx, hy = [], []
    for _ in range(10):
        x += 20; y += 920
        hx.append(x); hy.append(y)
    return cat(a, mk(hx, hy), diag(300, x0=x + 10, y0=y + 10))


def backtrack_cases():
    out = [Case(f"interleave_{d}", "interleave_70" if d == 70 else "backtrack", [interleaved(d)]) for d in (2, 63, 70)]
    # score exactly min_chain_score - 1 / min_chain_score; min_cnt - 1 / min_cnt anchors
    out.append(Case("min_score_edge", "backtrack", [diag_steps([10, 10]), diag_steps([10, 11])], pins=dict(n_chains=[0, 1])))
    out.append(Case("min_cnt_edge", "backtrack", [diag(2, step=30, span=40), diag(3, step=30, span=40)], pins=dict(n_chains=[0, 1])))
    out.append(Case("max_drop", "backtrack", [max_drop_chain()], pins=dict(n_chains=[2])))
    # the hops take 1 220 off the running maximum: max_drop (= bw) of 1 219 cuts the chain there, 1 220 is not exceeded and the chain runs through
    out.append(Case("max_drop_1219", "backtrack", [max_drop_chain()], replace(ASM10, bw=1219), pins=dict(n_chains=[2])))
    out.append(Case("max_drop_1220", "backtrack", [max_drop_chain()], replace(ASM10, bw=1220), pins=dict(n_chains=[1])))
    return out


# ------------------------------------------------------------------------------------------------ equal candidate scores
EQUAL_COUNTS = (2, 3, 64, 65, 300)


def equal_score_cases():
    out = []
    # c identical 8-anchor chains on c targets: candidates of equal score, distinct keys in compact_a's sort (insertion sort up to 64 chains, radix above)
    out.append(Case("equal_targets", "equal_targets", [cat(*[diag(8, rid=r) for r in range(c)]) for c in EQUAL_COUNTS], pins=dict(n_chains=list(EQUAL_COUNTS))))
    # the same with every chain starting at the same target position (equal keys in compact_a's sort): one target, the query positions 20 000 apart
    out.append(Case("equal_starts", "equal_starts", [cat(*[diag(8, y0=500 + 20_000 * m) for m in range(c)]) for c in EQUAL_COUNTS], pins=dict(n_chains=list(EQUAL_COUNTS))))
    # two chains of equal score that share a trunk: the second walk stops at a mark of its own score
    fork = cat(diag(20, x0=1000, y0=1000), diag(12, x0=1200, y0=1240), diag(12, x0=1240, y0=1200))
    out.append(Case("equal_fork", "equal_fork", [fork]))
    return out


def all_cases():
    cases = (colinear_cases() + [bound_case(), y_range_edge_case(), inner_y_edge_case()] + overflow_cases() + cap_cases() + tie_cases() + summary_cases() + [evicted_minimum_case()] + grid_cases() + wrap_cases() + [equal_x_case()] + segmentation_cases()
             + sort_edge_cases() + backtrack_cases() + equal_score_cases())
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


def groups():
    out = {}
    for c in all_cases():
        out.setdefault(c.group, []).append(c)
    return out


def free_of_order_ties(query, f, params):
    """no two candidate chain ends (f >= min_chain_score) of the query score alike and no two of its anchors share x: nothing the reference's
    unstable sorts could arrange differently"""
    cand = np.asarray(f)[np.asarray(f) >= params.min_chain_score]
    return len(np.unique(cand)) == len(cand) and len(np.unique(query[:, 0])) == len(query)
