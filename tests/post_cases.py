"""Cases for the post-DP kernels (pangraph_amd/csrc/pga_post.hip), built on purpose: the end-to-end genomes of the suite (uniform random bases,
0.4-3 % divergence) never slide an indel past one ballot, never swallow a match run, never emit I D I, and put no event on a trip or lane edge.

A finish case is (target codes, ALIGNED-STRAND query codes, operation list): the region spans both sequences.  The GPU test derives the forward
query for q_rev = 1 and embeds both windows at offsets (VARIANTS).  Every case names the properties it exists for as `pins`;
tests/test_post_cases_cpu.py asserts them from the compiled reference's answer alone, so a case that no longer reaches its edge fails there.
Pins that depend on the scoring are evaluated under PIN_SC.

  pins: final (the reference's final list, as a string), qs / rs (its shifts), n_final (its final n_cigar), squeezed (the list got shorter and
        holds no empty operation), s_zero (the running score hits the clamp inside a match run after having been positive), frac (the running
        score enters a match run with a fractional part), n_ambi (> 0), dp_max (its value under PIN_SC)

Pure numpy, fixed seeds, no GPU.
"""
from dataclasses import dataclass, field

import numpy as np

# (a, b, q, e) with sc_ambi 1: the three presets, one with a = 2, one with a = 0 (the position-by-position branch of the running score)
SCORINGS = ((1, 19, 39, 3), (1, 9, 16, 2), (1, 4, 6, 2), (2, 4, 4, 2), (0, 4, 6, 2))
PIN_SC = SCORINGS[0]
# the second gap cost of each scoring (q2, e2), for the host shortcut: the presets' own, the others' made up in their proportion
DUAL = {(1, 19, 39, 3): (81, 1), (1, 9, 16, 2): (41, 1), (1, 4, 6, 2): (26, 1), (2, 4, 4, 2): (24, 1), (0, 4, 6, 2): (26, 1)}
# how the GPU test embeds a case: (q_rev, bases in front of / behind the query window on the aligned strand, in front of / behind the target
# window).  With q_rev = 1 the pad behind the window is the forward position its last base lands on: 0 and 9 reach the branch for the start of
# the store when the case is request 0
VARIANTS = ((0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (0, 5, 7, 33, 3), (1, 19, 9, 21, 0))
FIN_LDS_OPS = 6144
OPS = "MIDN"


@dataclass
class Case:
    name: str
    family: str
    t: np.ndarray
    q: np.ndarray                       # on the aligned strand
    cigar: np.ndarray                   # uint32, length << 4 | op
    pins: dict = field(default_factory=dict)


def cig(s):
    """'20M3I5D' -> uint32 array"""
    out, num = [], ""
    for ch in s:
        if ch.isdigit():
            num += ch
        else:
            out.append(int(num) << 4 | OPS.index(ch))
            num = ""
    return np.array(out, dtype=np.uint32)


def cigstr(c):
    return "".join(f"{int(x) >> 4}{OPS[int(x) & 0xf]}" for x in c)


def spans(c):
    """(query span, target span) of a list"""
    c = np.asarray(c, np.int64)
    op, ln = c & 0xf, c >> 4
    return int(ln[(op == 0) | (op == 1)].sum()), int(ln[(op == 0) | (op == 2) | (op == 3)].sum())


def rand(rng, n, alphabet=4):
    return rng.integers(0, alphabet, n).astype(np.uint8)


def cat(*parts):
    return np.concatenate([np.asarray(p, np.uint8) for p in parts]).astype(np.uint8)


def derive_q(t, c, rng, ins=None):
    """the query a list implies over a target: match runs copy the target, insertions take `ins` (an iterator of arrays) or random bases"""
    out, i = [], 0
    for x in c:
        op, ln = int(x) & 0xf, int(x) >> 4
        if op == 0:
            out.append(t[i:i + ln]); i += ln
        elif op == 1:
            out.append(next(ins) if ins is not None else rand(rng, ln))
        else:
            i += ln
    assert i == len(t)
    return cat(*out) if out else np.zeros(0, np.uint8)


def mutate(seq, pos, rng=None):
    """another base at every position of pos (deterministic: base + 1 mod 4; N becomes 0)"""
    s = seq.copy()
    p = np.asarray(pos, np.int64)
    s[p] = np.where(s[p] > 3, 0, (s[p] + 1) & 3)
    return s


# ------------------------------------------------------------------------------------------------ slides
UNITS = {"hp": [0], "p2": [0, 1], "p3": [0, 1, 2]}
SLIDES = (1, 63, 64, 65, 128, 200)


def _periodic(unit, n):
    return np.resize(np.array(unit, np.uint8), n) if n else np.zeros(0, np.uint8)


def slide_case(kind, uname, k, pre, rng, tail=12):
    """an indel of one repeat period (3 for the homopolymer) right behind k repeat bases, behind `pre` bases that end in a base outside the repeat: it
    slides k bases and stops; pre == 0: the slide takes the whole run in front (slid == room), the indel becomes the first operation and is cut"""
    unit = UNITS[uname]
    ln = {"hp": 3, "p2": 4, "p3": 3}[uname]
    flank = cat(rand(rng, pre - 1), [3]) if pre else np.zeros(0, np.uint8)
    right = cat([3], rand(rng, 20))
    rep = _periodic(unit, k + ln + tail)
    longer = cat(flank, rep, right)
    shorter = cat(flank, rep[:k], rep[k + ln:], right)           # continues the period across the indel: the run behind the indel matches
    q, t = (longer, shorter) if kind == "I" else (shorter, longer)
    c = cig(f"{pre + k}M{ln}{kind}{tail + 21}M")
    if pre:
        pins = dict(final=f"{pre}M{ln}{kind}{k + tail + 21}M", qs=0, rs=0)
    else:
        pins = dict(final=f"{k + tail + 21}M", qs=ln if kind == "I" else 0, rs=ln if kind == "D" else 0, squeezed=True)
    return Case(f"slide_{kind}_{uname}_{k}_{'stop' if pre else 'room'}", "slides", t, q, c, pins)


def slide_cases():
    rng = np.random.default_rng(101)
    out = []
    for kind in "ID":
        for uname in UNITS:
            for k in SLIDES:
                out.append(slide_case(kind, uname, k, 7, rng))
                out.append(slide_case(kind, uname, k, 0, rng))
    A = lambda n: np.zeros(n, np.uint8)
    out.append(Case("slide_polyA_5M3I20M", "slides", A(25), A(28), cig("5M3I20M"), dict(final="25M", qs=3, rs=0, squeezed=True)))
    out.append(Case("slide_del_150_into_200", "slides", cat([1, 2, 3], A(210)), cat([1, 2, 3], A(200)), cig("153M10D50M"), dict(final="3M10D200M", qs=0, rs=0)))
    # an indel next to another indel, first or last in the list: no slide, though the bases would allow one
    out.append(Case("slide_none_adjacent", "slides", A(63), A(62), cig("30M2I3D30M"), dict(final="30M2I3D30M", qs=0, rs=0)))
    out.append(Case("slide_none_first", "slides", A(30), A(33), cig("3I30M"), dict(final="30M", qs=3, rs=0)))
    out.append(Case("slide_none_last", "slides", A(30), A(33), cig("30M3I"), dict(final="30M3I", qs=0, rs=0)))
    # two slides in a row: the first lengthens the run in front of the second, which slides further than its own run was long
    f = np.array([1, 2, 1, 2, 3], np.uint8)
    q = cat(f, A(30 + 2 + 10 + 20))
    t = cat(f, A(10), [1], A(19), A(10), A(3), A(20))
    out.append(Case("slide_two_in_a_row", "slides", t, q, cig("35M2I10M3D20M"), dict(final="5M2I11M3D49M", qs=0, rs=0)))
    # ... and takes all of it: the run between them is squeezed out and the two indels meet
    t = cat(f, A(30 + 10 + 3 + 20))
    out.append(Case("slide_two_in_a_row_room", "slides", t, q, cig("35M2I10M3D20M"), dict(final="5M2I3D60M", qs=0, rs=0, squeezed=True)))
    return out


# ------------------------------------------------------------------------------------------------ merges, leading indels
def _plain(name, family, s, rng, pins, alphabet=4):
    c = cig(s)
    t = rand(rng, spans(c)[1], alphabet)
    return Case(name, family, t, derive_q(t, c, rng), c, pins)


def merge_cases():
    rng = np.random.default_rng(202)
    rows = [("IDI", "20M3I5D4I35M", dict(final="20M7I5D35M", squeezed=True)),
            ("DIDI", "20M2D3I4D1I30M", dict(final="20M4I6D30M", squeezed=True)),
            ("ID_alone", "20M3I5D30M", dict(final="20M3I5D30M")),
            ("DI_alone", "20M5D3I30M", dict(final="20M5D3I30M")),
            ("zero_front", "20M0I3I5D4I30M", dict(final="20M7I5D30M", squeezed=True)),
            ("zero_front_D", "20M0D3I5D4I30M", dict(final="20M7I5D30M", squeezed=True)),
            ("zero_middle", "20M3I5D0M4I30M", dict(final="20M7I5D30M", squeezed=True)),
            ("zero_end", "20M3I5D4I0D30M", dict(final="20M7I5D30M", squeezed=True)),
            ("zero_only", "20M0I30M", dict(final="50M", squeezed=True)),
            ("start_IDI", "3I5D4I35M", dict(final="5D35M", qs=7, rs=0, squeezed=True)),
            ("start_DID", "2D3I4D30M", dict(final="6D30M", qs=3, rs=0, squeezed=True)),
            ("start_zero_IDI", "0M3I5D4I35M", dict(final="5D35M", qs=7, rs=0, squeezed=True)),
            ("end_IDI", "35M3I5D4I", dict(final="35M7I5D", squeezed=True)),
            ("two_stretches", "10M1I2D3I10M4D5I6D10M", dict(final="10M4I2D10M5I10D10M", squeezed=True)),
            ("all_indel", "3I5D4I", dict(final="5D", qs=7, rs=0, squeezed=True))]
    return [_plain(f"merge_{n}", "merges", s, rng, p) for n, s, p in rows]


def leading_cases():
    rng = np.random.default_rng(303)
    rows = [("I", "4I30M", dict(final="30M", qs=4, rs=0)), ("D", "4D30M", dict(final="30M", qs=0, rs=4)),
            ("I_long", "100I30M", dict(final="30M", qs=100, rs=0)), ("D_then_I", "4D3I30M", dict(final="3I30M", qs=0, rs=4)),
            ("one_M", "30M", dict(final="30M", qs=0, rs=0)), ("one_I", "5I", dict(final="5I", qs=0, rs=0)), ("one_D", "5D", dict(final="5D", qs=0, rs=0)),
            ("one_M_1", "1M", dict(final="1M", qs=0, rs=0)), ("N_skip", "20M50N20M", dict(final="20M50N20M")), ("N_first", "7N20M", dict(final="7N20M", qs=0, rs=0))]
    return [_plain(f"leading_{n}", "leading", s, rng, p) for n, s, p in rows]


# ------------------------------------------------------------------------------------------------ match runs: trip and lane edges
RUNS = (1, 15, 16, 17, 1023, 1024, 1025, 2047, 2049, 5000)
EDGES = (0, 15, 16, 1023, 1024)


def run_cases():
    rng = np.random.default_rng(404)
    out = []
    for L in RUNS:
        t = rand(rng, L)
        out.append(Case(f"run_{L}_clean", "runs", t, t.copy(), cig(f"{L}M"), dict(final=f"{L}M")))
        for pos in sorted(set(p for p in EDGES + (L - 1,) if p < L)):
            out.append(Case(f"run_{L}_mis_{pos}", "runs", t, mutate(t, [pos]), cig(f"{L}M")))
            qn = t.copy(); qn[pos] = 4
            out.append(Case(f"run_{L}_Nq_{pos}", "runs", t, qn, cig(f"{L}M"), dict(n_ambi=True)))
            out.append(Case(f"run_{L}_Nt_{pos}", "runs", qn, t.copy(), cig(f"{L}M"), dict(n_ambi=True)))
            # the same event in a run that a gap precedes: s enters the run with the fractional part of e * log2(1 + len)
            c = cig(f"60M3D{L}M2I9M")
            t2 = cat(rand(rng, 63), t, rand(rng, 9))
            ins = np.array([rng.integers(0, 4), (int(t[-1]) + 2) & 3], np.uint8)         # differs from the run's last base, mutated or not: the insertion stays
            q2 = derive_q(t2, c, rng, ins=iter([ins]))
            q2 = mutate(q2, [60 + pos])
            out.append(Case(f"run_{L}_gap_mis_{pos}", "runs", t2, q2, c, dict(frac=True)))
    # bursts of mismatches that take s to zero inside a trip, after which it recovers
    for L, start, n in ((300, 10, 3), (1500, 200, 40), (1500, 1100, 40), (2049, 14, 3), (2049, 1030, 12), (5000, 1024, 40), (5000, 15, 17)):
        t = rand(rng, L)
        q = mutate(t, np.arange(start, start + n))
        if start > 19 * n - 30:                 # not enough on its own under PIN_SC: an earlier burst takes s down first
            q = mutate(q, np.arange(max(0, start - 30 - (start + 18) // 19), start - 30))
        out.append(Case(f"run_{L}_burst_{start}_{n}", "runs", t, q, cig(f"{L}M"), dict(s_zero=True)))
    # a burst across the trip edge at base 1024 that reaches zero behind it
    t = rand(rng, 2049)
    q = mutate(mutate(t, np.arange(900, 960)), np.arange(1010, 1040))
    out.append(Case("run_2049_burst_straddle", "runs", t, q, cig("2049M"), dict(s_zero=True)))
    c = cig("80M2I2049M")
    t2 = cat(rand(rng, 80), t)
    q2 = cat(t2[:80], rand(rng, 2), q)
    out.append(Case("run_2049_burst_straddle_gap", "runs", t2, q2, c, dict(s_zero=True, frac=True)))
    for L in (17, 1025):
        t = rand(rng, L)
        out.append(Case(f"run_{L}_all_N_q", "runs", t, np.full(L, 4, np.uint8), cig(f"{L}M"), dict(n_ambi=True)))
        out.append(Case(f"run_{L}_all_N_both", "runs", np.full(L, 4, np.uint8), np.full(L, 4, np.uint8), cig(f"{L}M"), dict(n_ambi=True)))
    t = rand(rng, 60)
    out.append(Case("run_N_in_gaps", "runs", cat(t[:20], [4, 4, 0], t[20:]), cat(t[:40], [4, 1], t[40:]), cig("20M3D20M2I20M"), dict(n_ambi=True)))
    return out


# ------------------------------------------------------------------------------------------------ peaks: the maximum inside a trip, behind a clamp
def peak_cases():
    """One run: d bad columns (mismatches, or N in the query for odd lanes) that hold s at zero, clean bases up to in-trip position 16 * lane + r, then 40
    mismatches to the end.  The maximum of the whole list is s at that position: the block form finds it as max(P - pmin) in that lane with the
    prefix minimum handed over from the lanes in front -- every lane of the first trip (d = 3) and of the second (d = 1030: the clamp is taken inside
    the second trip), r between the first base a lane can see behind the clamp and its last (r = 15: the maximum is the lane's closing position)"""
    rng = np.random.default_rng(1111)
    out = []
    for d, r0, rn in ((3, 4, 12), (1030, 7, 9)):
        for lane in range(64):
            peak = d // 1024 * 1024 + 16 * lane + r0 + (5 * lane) % rn           # the last clean base
            L = peak + 1 + 40
            t = rand(rng, L)
            q = mutate(t, np.concatenate([np.arange(d), np.arange(peak + 1, L)]))
            if lane & 1:
                q[:d] = 4
            out.append(Case(f"peak_{d}_lane{lane}_{peak % 16}", "peaks", t, q, cig(f"{L}M"), dict(dp_max=peak + 1 - d, final=f"{L}M")))
    return out


# ------------------------------------------------------------------------------------------------ long lists: LDS or in place in HBM
def _long(name, n_units, rng, lead, tail_m, slide):
    """(2M1I) x n_units [+ 2M], optionally behind a leading 1I.  slide = False: every inserted base differs from the base in front of
    it, so nothing slides or fuses and the final list is the input list less the leading indel"""
    t = rand(rng, 2 * n_units + (2 if tail_m else 0))
    q = np.zeros(3 * n_units + (2 if tail_m else 0) + (1 if lead else 0), np.uint8)
    body = q[1:] if lead else q
    u = body[:3 * n_units].reshape(n_units, 3)
    u[:, :2] = t[:2 * n_units].reshape(n_units, 2)
    if slide:
        u[:, 2] = rand(rng, n_units)
    else:
        u[:, 2] = (u[:, 1] + 1 + rng.integers(0, 2, n_units)) & 3                  # differs from the base in front
    if tail_m:
        body[3 * n_units:] = t[2 * n_units:]
    if lead:
        q[0] = rng.integers(0, 4)
    c = np.tile(cig("2M1I"), n_units)
    c = np.concatenate(([cig("1I")] if lead else []) + [c] + ([cig("2M")] if tail_m else [])).astype(np.uint32)
    n_in = len(c)
    pins = dict(qs=1 if lead else 0, rs=0) if not slide else {}
    if not slide:
        pins["n_final"] = n_in - (1 if lead else 0)
    return Case(name, "long_lists", t, q, c, pins)


def long_list_cases():
    rng = np.random.default_rng(505)
    out = [_long("long_6143", 3071, rng, False, True, False), _long("long_6144", 3072, rng, False, False, False), _long("long_6145", 3072, rng, False, True, False),
           _long("long_7001", 3500, rng, False, True, False),
           # with a leading indel: the input has one operation more than the final list (6144 in: LDS; 6145, 6146 and 7002 in: in place in HBM)
           _long("long_lead_6143", 3071, rng, True, True, False), _long("long_lead_6144", 3072, rng, True, False, False),
           _long("long_lead_6145", 3072, rng, True, True, False), _long("long_lead_7001", 3500, rng, True, True, False),
           # random inserted bases: about a tenth of the insertions slide into their neighbours and fuse
           _long("long_random_7000", 3500, rng, False, False, True), _long("long_lead_random_7001", 3500, rng, True, False, True)]
    out[-2].pins["n_final_gt"] = FIN_LDS_OPS
    out[-1].pins["n_final_gt"] = FIN_LDS_OPS
    return out


# ------------------------------------------------------------------------------------------------ random lists
def random_case(name, family, rng, n_ops_max=60, len_max=40):
    n_ops = int(rng.integers(1, n_ops_max + 1))
    with_n = rng.random() < 0.2
    alphabet = int(rng.choice([2, 3, 4, 4]))                                     # small alphabets: indels slide often
    ops, prev = [], -1
    for _ in range(n_ops):
        op = int(rng.choice([0, 0, 0, 1, 2, 3] if with_n else [0, 0, 0, 1, 2]))
        if op == prev and rng.random() < 0.9:
            op = (op + 1) % 3
        ln = 0 if rng.random() < 0.03 else int(rng.integers(1, len_max + 1)) if op == 0 else int(rng.integers(1, 12))
        ops.append(ln << 4 | op); prev = op
    c = np.array(ops, np.uint32)
    qs, ts = spans(c)
    t = rand(rng, ts, alphabet)
    q = derive_q(t, c, rng, ins=iter([rand(rng, int(x) >> 4, alphabet) for x in c if int(x) & 0xf == 1]))
    mis, amb = rng.random() * 0.3, rng.random() * 0.03
    if len(q):
        q = mutate(q, np.nonzero(rng.random(len(q)) < mis)[0])
        q[rng.random(len(q)) < amb] = 4
    if len(t):
        t = t.copy(); t[rng.random(len(t)) < amb / 2] = 4
    return Case(name, family, t, q, c)


def random_cases(n=300):
    rng = np.random.default_rng(606)
    return [random_case(f"random_{i}", "random", rng) for i in range(n)]


# ------------------------------------------------------------------------------------------------ batches: the device-buffer route, LDS reuse
def batch_pools():
    """two pools of tiny cases: A with lists of 1-3 operations, B (different seed, different shape) with lists of 5-9"""
    rng = np.random.default_rng(707)
    A = [random_case(f"tinyA_{i}", "batches", rng, n_ops_max=3, len_max=12) for i in range(64)]
    B = []
    while len(B) < 8:
        c = random_case(f"tinyB_{len(B)}", "batches", rng, n_ops_max=9, len_max=30)
        if len(c.cigar) >= 5:
            B.append(c)
    return A, B


def batches():
    """name -> list of cases (one request each).  4097: just over the pinned-memory route.  8200: the grid has 8192 waves, so requests 8192.. run
    on waves that finished one of the first 8192 in the same LDS; they come from pool B: other cases, longer lists than their predecessors"""
    A, B = batch_pools()
    return {"batch_4097": [A[i % len(A)] for i in range(4097)],
            "batch_8200": [A[(i * 7) % len(A)] for i in range(8192)] + B}


# ------------------------------------------------------------------------------------------------ the first sequence of the store
def first_in_store_cases():
    """cases whose last match run ends on the last base of the query window: with q_rev = 1 and r bases behind the window (r = 0..14) that run ends on
    forward position r of the query, below which the sixteen-base read has its own branch when the query is the first sequence of the store"""
    rng = np.random.default_rng(808)
    out = []
    for s in ("40M", "20M2I30M", "5M1D9M", "3M", "17M4D1040M"):
        c = _plain(f"first_{s}", "first_in_store", s, rng, {})
        c.q = mutate(c.q, [len(c.q) - 1 - k for k in (0, 2) if k < len(c.q)])
        out.append(c)
    t = rand(rng, 31); q = t.copy(); q[[30, 17, 15, 14]] = 4
    out.append(Case("first_N_31M", "first_in_store", t, q, cig("31M"), dict(n_ambi=True)))
    return out


FAMILIES = ("slides", "merges", "leading", "runs", "peaks", "long_lists", "random", "first_in_store")


def all_cases():
    """every finish case outside the batches"""
    return slide_cases() + merge_cases() + leading_cases() + run_cases() + peak_cases() + long_list_cases() + random_cases() + first_in_store_cases()


# ------------------------------------------------------------------------------------------------ identity probes
PROBE_LENGTHS = (1, 63, 64, 65, 200, 3000)
PROBE_M_MAX = 5


def probe_cases():
    """(name, target window, aligned-strand query window, expected answer): 0, m_max and m_max + 1 mismatches, the last mismatch in the last 64-base
    block, an N in the first and in the last block"""
    rng = np.random.default_rng(909)
    out = []
    for n in PROBE_LENGTHS:
        t = rand(rng, n)
        last0 = (n - 1) // 64 * 64
        for m in (0, PROBE_M_MAX, PROBE_M_MAX + 1):
            m = min(m, n)
            pos = np.sort(rng.choice(n, m, replace=False)) if m else np.zeros(0, np.int64)
            out.append((f"probe_{n}_m{m}", t, mutate(t, pos), m if m <= PROBE_M_MAX else -1))
            if m:
                k = min(m - 1, n - 1)
                pos2 = np.concatenate([rng.choice(n - 1, k, replace=False) if k else np.zeros(0, np.int64), [n - 1]]).astype(np.int64)
                out.append((f"probe_{n}_m{m}_last_block", t, mutate(t, pos2), len(pos2) if len(pos2) <= PROBE_M_MAX else -1))
        for where, p in (("first", min(3, n - 1)), ("last", n - 1), ("last_block_start", last0)):
            qn = t.copy(); qn[p] = 4
            out.append((f"probe_{n}_Nq_{where}", t, qn, -1))
            out.append((f"probe_{n}_Nt_{where}", qn, t.copy(), -1))
    return out


def probe_batch(n=33_000):
    """more probes than the grid has waves (32 768): (target windows, query windows) as two (n, 8) arrays; about a third differ in 1-3 bases"""
    rng = np.random.default_rng(1010)
    t = rand(rng, n * 8).reshape(n, 8)
    q = t.copy()
    hit = rng.random((n, 8)) < 0.06
    q[hit] = (q[hit] + 1) & 3
    q[rng.random((n, 8)) < 0.002] = 4
    return t, q
