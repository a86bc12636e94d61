"""Inputs for pga_close_round (pangraph_amd/close.py) and the expectation they are held against.  The entry is a pure function of its inputs,
so a case is a SPEC: a dict graph in the shape of tests/simplify_ref.py (blocks {id: {"consensus", "alignments": {node id: edit}}}, nodes,
paths), the ids of the updated ("merged") blocks, and per updated block what a reconsensus is said to have returned -- its kind, its
consensus and the edits of the members the first detach kept.  Who leaves a block is decided by the edits themselves: a member whose
deletions sum to the consensus length is unaligned (tests/detach_ref.py).  `build` runs detach_ref.expected_call on the merged-only blocks
and on the invented blocks behind the reconsensus: those two results are the `detached` / `redetached` of the call.

`host_close` is the other route to the same end: the dict graph after detach_ref.detach_unaligned_nodes, the replacement of the updated
blocks, and detach_unaligned_nodes on the kind-2 blocks only (as the reference runs it), flattened in ascending block id, within a block in
ascending node id.  It never reads a member_map.  `flat_close` restates the header's text with loops over the tables, index after index;
it stands in for the call where there is no device.
A case is {"t": the tables of close.Tables, "exp": what CloseOut.to_lists() gives, "spec", "after": host_close's dict graph}."""
import copy
import functools

import numpy as np

import detach_ref as dr
from pangraph_amd.close import NONE, TILE
from pangraph_amd.detach import DEL, INS, SUB

LETTERS = "ACGT"


def edit(subs=(), dels=(), inss=()):
    return {"subs": list(subs), "dels": list(dels), "inss": list(inss)}


def random_edit(rng, cons_len, n=None):
    """a member that stays: its deletions never cover the consensus"""
    n = n if n is not None else [int(x) for x in rng.choice([0, 0, 1, 2, 5], 3)]
    return edit([(int(rng.integers(0, max(cons_len, 1))), LETTERS[int(rng.integers(0, 4))]) for _ in range(n[0])],
                [(int(rng.integers(0, max(cons_len, 1))), 0) for _ in range(n[1])],
                [(int(rng.integers(0, cons_len + 1)), "".join(LETTERS[int(x)] for x in rng.integers(0, 4, int(rng.integers(0, 9))))) for _ in range(n[2])])


def unaligned(cons_len, inss=()):
    """a member that leaves: one deletion over the whole consensus; its sequence is what it inserts"""
    return edit([], [(0, cons_len)] if cons_len else [], inss)


# ---------------------------------------------------------------- flattening
class _Pool:
    """insertion letters placed in one buffer: a sequence that is already there is shared (so offsets repeat and overlap), and the
    insertions are placed in a shuffled order (so offsets do not ascend)"""

    def __init__(self, rng):
        self.rng, self.buf = rng, bytearray()

    def place(self, seqs):
        at = [0] * len(seqs)
        for k in self.rng.permutation(len(seqs)):
            s = seqs[k].encode("latin-1")
            found = bytes(self.buf).find(s) if len(s) < 64 else -1
            if found < 0 or not s:
                found = len(self.buf) if s else int(self.rng.integers(0, len(self.buf) + 1))
                self.buf += s
            at[k] = found
        return at


def flat_edits(edits, pool):
    """edits in member order -> (counts, subs, dels, inss) with seq_off into pool.buf"""
    counts = np.array([[len(e["subs"]), len(e["dels"]), len(e["inss"])] for e in edits], np.uint32).reshape(-1, 3)
    subs = np.array([(p, ord(a)) for e in edits for p, a in e["subs"]], SUB) if counts[:, 0].sum() else np.zeros(0, SUB)
    dels = np.array([tuple(d) for e in edits for d in e["dels"]], DEL) if counts[:, 1].sum() else np.zeros(0, DEL)
    seqs = [s for e in edits for _, s in e["inss"]]
    at = pool.place(seqs)
    inss = np.array([(p, len(s), at[k]) for k, (p, s) in enumerate((p, s) for e in edits for p, s in e["inss"])], INS) if seqs else np.zeros(0, INS)
    return counts, subs, dels, inss


def graph_lists(g, dead=()):
    """-> (blocks, paths, nodes, order): the flat graph with the dead entries given ({id: anything}) between the alive ones"""
    bids = sorted(set(g["blocks"]) | set(dead))
    order = {b: sorted(g["blocks"][b]["alignments"]) if b in g["blocks"] else [] for b in bids}
    at = {b: i for i, b in enumerate(bids)}
    slot = {n: k for b in bids for k, n in enumerate(order[b])}
    blocks = [(b, len(g["blocks"][b]["consensus"]), len(order[b]), 1) if b in g["blocks"] else (b, 0, 0, 0) for b in bids]
    paths, nodes = [], []
    for pid in sorted(g["paths"]):
        p = g["paths"][pid]
        paths.append((pid, len(nodes), len(p["nodes"]), int(bool(p["circular"]))))
        nodes += [(n, g["nodes"][n]["position"][0], g["nodes"][n]["position"][1], at[g["nodes"][n]["block_id"]], slot[n], int(g["nodes"][n]["strand"] == "-")) for n in p["nodes"]]
    return blocks, paths, nodes, order


# ---------------------------------------------------------------- the expectation: the dict route
class Conflict(Exception):
    """the reference panics "Conflicting key" """


def host_close(spec):
    """-> the dict graph after the tail of the round"""
    g = copy.deepcopy({k: spec[k] for k in ("blocks", "nodes", "paths")})
    upd = list(spec["upd"])

    def detach(ids):
        blocks = [(b, g["blocks"][b]) for b in ids]
        dr.detach_unaligned_nodes(blocks, g["nodes"])
        for bid, blk in blocks[len(ids):]:
            if bid in g["blocks"]:
                raise Conflict(bid)
            g["blocks"][bid] = blk

    detach(upd)
    for b in upd:
        kind, cons, edits = spec["rc"][b]
        assert sorted(edits) == sorted(g["blocks"][b]["alignments"]), "the spec's reconsensus covers the members the first detach kept"
        g["blocks"][b] = {"consensus": cons, "alignments": {n: copy.deepcopy(e) for n, e in edits.items()}}
    detach([b for b in upd if spec["rc"][b][0] == 2])
    return g


def flatten(spec, after, orphan_rows):
    """the dict graph after -> what CloseOut.to_lists() gives; orphan_rows: [(node_id, block_id, len)] in record order"""
    blocks, paths, nodes, order = graph_lists(after)
    before_blocks, _, _, before_order = graph_lists(spec, spec.get("dead", ()))
    member_before, m = {}, 0
    for b, _, _, alive in before_blocks:
        for n in before_order[b]:
            member_before[n] = m
            m += 1
    at = {b[0]: i for i, b in enumerate(blocks)}
    edits = [after["blocks"][b[0]]["alignments"][n] for b in blocks for n in order[b[0]]]
    counts = np.array([[len(e["subs"]), len(e["dels"]), len(e["inss"])] for e in edits], np.uint32).reshape(-1, 3)
    subs = np.array([(p, ord(a)) for e in edits for p, a in e["subs"]], SUB) if counts[:, 0].sum() else np.zeros(0, SUB)
    dels = np.array([tuple(d) for e in edits for d in e["dels"]], DEL) if counts[:, 1].sum() else np.zeros(0, DEL)
    letters, rows = bytearray(), []
    for e in edits:
        for p, s in e["inss"]:
            rows.append((p, len(s), len(letters)))
            letters += s.encode("latin-1")
    inss = np.array(rows, INS) if rows else np.zeros(0, INS)
    who = [(n, int(after["nodes"][n]["strand"] == "-")) for b in blocks for n in order[b[0]]]
    return {"blocks": blocks, "paths": paths, "nodes": nodes, "rc_blocks": [(after["blocks"][b[0]]["consensus"].encode("latin-1"), b[2]) for b in blocks],
            "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": bytes(letters), "who": who, "origin": [member_before[n] for n, _ in who],
            "block_map": [at[b[0]] if b[3] else NONE for b in before_blocks], "kinds": [spec["rc"][b][0] for b in spec["upd"]],
            "orphans": [(member_before[n], n, bid, at[bid], ln, 0) for n, bid, ln in orphan_rows],
            "totals": (len(blocks), len(paths), len(nodes), len(who), len(orphan_rows), len(subs), len(dels), len(inss), len(letters))}


# ---------------------------------------------------------------- the tables of the call
def build(spec, seed=0):
    rng = np.random.default_rng(7000 + seed)
    blocks, paths, nodes, order = graph_lists(spec, spec.get("dead", ()))
    g = spec
    pool = _Pool(rng)
    pool.buf += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 50))
    counts, subs, dels, inss = flat_edits([g["blocks"][b[0]]["alignments"][n] for b in blocks for n in order[b[0]]], pool)
    at = {b[0]: i for i, b in enumerate(blocks)}
    upd = list(spec["upd"])
    merged = [{"consensus": g["blocks"][b]["consensus"], "members": [g["blocks"][b]["alignments"][n] for n in order[b]]} for b in upd]
    who_m = [[(n, g["nodes"][n]["strand"] == "-") for n in order[b]] for b in upd]
    d1 = dr.expected_call(merged, who_m)
    flat_ids = [n for b in upd for n in order[b]]
    gone = {o["member"] for o in d1["orphans"]}
    pos = {n: i for i, n in enumerate(flat_ids)}
    kept_ids = [[n for n in order[b] if pos[n] not in gone] for b in upd]
    blocks2 = [{"consensus": spec["rc"][b][1], "members": [spec["rc"][b][2][n] for n in ids]} for b, ids in zip(upd, kept_ids)]
    who2 = [[(n, g["nodes"][n]["strand"] == "-") for n in ids] for ids in kept_ids]
    d2 = dr.expected_call(blocks2, who2)
    flat2 = [n for ids in kept_ids for n in ids]
    for b, blk in zip(upd, d2["blocks"]):
        if spec["rc"][b][0] != 2:
            assert len(blk["members"]) == len(spec["rc"][b][2]), "only a realigned block loses members in the second detach"
    pool2 = _Pool(rng)
    pool2.buf += bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 30))
    counts2, subs2, dels2, inss2 = flat_edits([e for blk in d2["blocks"][:len(upd)] for e in blk["members"]], pool2)
    rows = lambda d: [(o["member"], o["node_id"], o["block_id"], o["len"], o["status"], (o["seq"] or "").encode("latin-1")) for o in d["orphans"]]
    t = {"blocks": blocks, "paths": paths, "nodes": nodes,
         "rc_blocks": [(g["blocks"][b[0]]["consensus"].encode("latin-1"), b[2]) if b[3] else (b"", 0) for b in blocks],
         "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": bytes(pool.buf),
         "who": [(n, int(g["nodes"][n]["strand"] == "-")) for b in blocks for n in order[b[0]]], "upd": [at[b] for b in upd]}
    if upd:
        t.update({"detached": {"n_members": [len(b["members"]) for b in d1["blocks"][:len(upd)]], "member_map": d1["member_map"], "orphans": rows(d1)},
                  "rc": {"blocks": [(spec["rc"][b][0], spec["rc"][b][1].encode("latin-1")) for b in upd], "status": [0] * len(flat2), "ins_seq": bytes(pool2.buf)},
                  "redetached": {"n_members": [len(b["members"]) for b in d2["blocks"][:len(upd)]], "member_map": d2["member_map"], "orphans": rows(d2),
                                 "counts": counts2, "subs": subs2, "dels": dels2, "inss": inss2}})
    after = host_close(spec)
    orphan_rows = [(o["node_id"], o["block_id"], o["len"]) for o in d1["orphans"]] + [(o["node_id"], o["block_id"], o["len"]) for o in d2["orphans"]]
    return {"t": t, "exp": flatten(spec, after, orphan_rows), "spec": spec, "after": after, "d1": d1, "d2": d2}


# ---------------------------------------------------------------- specs
def make_spec(rng, layout, upd, rc_of=None, leave1=lambda b, k: False, leave2=lambda b, k: False, kind_of=lambda b: 0, reverse=lambda b, k: False, ids=None,
              edit_of=None, orphan_ins=lambda b, k: [(0, "ACGTTGCA")], n_paths=3, dead=()):
    """layout: {block id: (cons_len, depth)}; upd: the updated ids; leave1 / leave2(block, k): member k (node-id order) leaves in the first / second stage;
    kind_of(block): the reconsensus kind; edit_of(rng, block, k, cons_len) -> an edit for a member that stays (before, and behind the reconsensus)"""
    edit_of = edit_of or (lambda rng, b, k, n: random_edit(rng, n))
    g = {"blocks": {}, "nodes": {}, "paths": {p: {"nodes": [], "circular": bool(p % 2), "tot_len": 1000, "name": f"p{p}"} for p in range(10, 10 + n_paths)}}
    nid = 100
    per_path = {p: 0 for p in g["paths"]}
    all_nodes = []
    for b in sorted(layout):
        cons_len, depth = layout[b]
        cons = "".join(LETTERS[int(x)] for x in rng.integers(0, 4, cons_len))
        aln = {}
        for k in range(depth):
            nid += int(rng.integers(1, 9))
            aln[nid] = unaligned(cons_len, orphan_ins(b, k)) if b in upd and leave1(b, k) else edit_of(rng, b, k, cons_len)
            p = sorted(g["paths"])[int(rng.integers(0, n_paths))] if not isinstance(ids, dict) or nid not in ids else ids[nid]
            g["nodes"][nid] = {"block_id": b, "path_id": p, "strand": "-" if reverse(b, k) else "+", "position": (per_path[p], per_path[p] + 7)}
            per_path[p] += 7
            all_nodes.append(nid)
        g["blocks"][b] = {"consensus": cons, "alignments": aln}
    for n in rng.permutation(all_nodes):
        g["paths"][g["nodes"][int(n)]["path_id"]]["nodes"].append(int(n))
    rc = {}
    for b in upd:
        cons_len = layout[b][0]
        kind = kind_of(b)
        kept = [(k, n) for k, n in enumerate(sorted(g["blocks"][b]["alignments"])) if not leave1(b, k)]
        if kind == 0:
            rc[b] = (0, g["blocks"][b]["consensus"], {n: copy.deepcopy(g["blocks"][b]["alignments"][n]) for _, n in kept})
        else:
            new_len = cons_len if kind == 1 else max(cons_len + int(rng.integers(-3, 4)), 1)
            cons = "".join(LETTERS[int(x)] for x in rng.integers(0, 4, new_len))
            rc[b] = (kind, cons, {n: unaligned(new_len, orphan_ins(b, k)) if kind == 2 and leave2(b, k) else edit_of(rng, b, k, new_len) for k, n in kept})
    return {"blocks": g["blocks"], "nodes": g["nodes"], "paths": g["paths"], "upd": sorted(upd), "rc": rc, "dead": {d: None for d in dead}}


def _small(seed, **kw):
    rng = np.random.default_rng(seed)
    layout = {50: (20, 3), 60: (30, 4), 70: (25, 5), 80: (10, 2), 90: (15, 0)}
    return build(make_spec(rng, layout, **kw), seed)


def _ids_case():
    """singleton ids below, between and above the survivors, up to 2^64 - 1: the ids are what detach_ref hashes, so the survivors are placed around them"""
    rng = np.random.default_rng(77)
    probe = make_spec(rng, {2: (20, 6)}, [2], leave1=lambda b, k: k < 3, leave2=lambda b, k: k == 4, kind_of=lambda b: 2, orphan_ins=lambda b, k: [(0, "ACGT" * (k + 1))])
    c = build(probe, 77)
    sing = sorted(o[2] for o in c["exp"]["orphans"])
    assert len(sing) == 4
    rng = np.random.default_rng(77)
    lo, hi = sing[0], sing[-1]
    layout = {2: (20, 6), lo + 1: (8, 1), (sing[1] + sing[2]) // 2: (9, 2), hi - 1: (5, 1)}
    if hi < (1 << 64) - 1:
        layout[(1 << 64) - 1] = (6, 1)
    spec = make_spec(rng, layout, [2], leave1=lambda b, k: k < 3, leave2=lambda b, k: k == 4, kind_of=lambda b: 2, orphan_ins=lambda b, k: [(0, "ACGT" * (k + 1))])
    c = build(spec, 77)
    assert sorted(o[2] for o in c["exp"]["orphans"]) == sing
    return c


def _tile(n, before=0):
    rng = np.random.default_rng(n)
    layout = {5: (6, before), 9: (12, n), 11: (7, 3)}
    return build(make_spec(rng, layout, [9], leave1=lambda b, k: k % 97 == 5, leave2=lambda b, k: k % 89 == 7, kind_of=lambda b: 2,
                           edit_of=lambda rng, b, k, m: random_edit(rng, m, (k % 3, k % 2, (k + 1) % 2))), n)


def _heavy(rng, b, k, n):
    if b == 9 and k == 700:
        return edit([(int(x), "A") for x in rng.integers(0, n, 5000)], [], [(int(x), "ACGT"[int(x) % 4] * (int(x) % 3)) for x in rng.integers(0, n, 3000)])
    return edit()


def _by_length(rng, b, k, n):
    return random_edit(rng, n, (k % 131, (k + 50) % 131, (k + 100) % 131))


INS_LETTERS = (0, 1, 63, 64, 65, 127, 128, 5000)


def _letters(rng, b, k, n):
    return edit([(0, "A")], [], [(int(rng.integers(0, n + 1)), "".join(LETTERS[int(x)] for x in rng.integers(0, 4, ln))) for ln in INS_LETTERS]) if k % 3 == 0 else random_edit(rng, n)


def _second_level(rng, b, k, n):
    return edit([(int(x) % n, "C") for x in range(TILE * TILE + 1)], [(0, 0)] * 3, [(0, "A"), (1, "")]) if (b, k) == (9, 1) else random_edit(rng, n, (2, 1, 1))


CASES = {
    "no_orphan": lambda: _small(1, upd=[50, 60, 70], kind_of=lambda b: {50: 0, 60: 1, 70: 2}[b]),
    "first_only": lambda: _small(2, upd=[60, 70], leave1=lambda b, k: k == 1, kind_of=lambda b: {60: 1, 70: 2}[b]),
    "second_only": lambda: _small(3, upd=[60, 70], leave2=lambda b, k: k in (0, 3), kind_of=lambda b: 2),
    "both_in_one_block": lambda: _small(4, upd=[70], leave1=lambda b, k: k in (0, 2), leave2=lambda b, k: k in (1, 4), kind_of=lambda b: 2),
    "block_loses_every_member": lambda: _small(5, upd=[50, 80], leave1=lambda b, k: b == 80 or k == 0, leave2=lambda b, k: b == 50, kind_of=lambda b: 2),
    "reverse_orphan": lambda: _small(6, upd=[60], leave1=lambda b, k: k == 2, reverse=lambda b, k: k in (1, 2), kind_of=lambda b: 0),
    "empty_orphan": lambda: _small(7, upd=[60, 70], leave1=lambda b, k: k == 0, leave2=lambda b, k: k == 2, kind_of=lambda b: 2, orphan_ins=lambda b, k: []),
    "id_ranges": _ids_case,
    "singleton_first": lambda: build(make_spec(np.random.default_rng(19), {(1 << 64) - 3: (20, 4), (1 << 64) - 2: (9, 2)}, [(1 << 64) - 3], leave1=lambda b, k: k == 1, leave2=lambda b, k: k == 2,
                                               kind_of=lambda b: 2), 19),
    "two_nodes_of_one_path": lambda: _small(8, upd=[70], leave1=lambda b, k: k in (1, 3), kind_of=lambda b: 1, n_paths=1),
    "dead_entries": lambda: _small(9, upd=[60], leave1=lambda b, k: k == 0, kind_of=lambda b: 2, dead=(40, 55, 65, 99)),
    "high_index": lambda: build(make_spec(np.random.default_rng(10), {**{b: (3, 1 if b % 7000 == 0 else 0) for b in range(1, 70001)}, 70001: (12, 4), 70002: (9, 2)}, [70001],
                                          leave1=lambda b, k: k == 1, leave2=lambda b, k: k == 3, kind_of=lambda b: 2, edit_of=lambda rng, b, k, n: random_edit(rng, n, (1, 0, 1))), 10),
    "members_1023": lambda: _tile(TILE - 1),
    "members_1024": lambda: _tile(TILE),
    "members_1025": lambda: _tile(TILE + 1),
    "straddle": lambda: _tile(100, before=1000),
    "one_heavy": lambda: build(make_spec(np.random.default_rng(13), {5: (6, 3), 9: (40, 2001), 11: (7, 2)}, [11], kind_of=lambda b: 1, edit_of=_heavy), 13),
    "one_heavy_updated": lambda: build(make_spec(np.random.default_rng(14), {5: (6, 3), 9: (40, 2001)}, [9], leave1=lambda b, k: k == 3, kind_of=lambda b: 2, edit_of=_heavy), 14),
    "list_lengths": lambda: build(make_spec(np.random.default_rng(15), {5: (200, 140), 9: (200, 140)}, [9], leave1=lambda b, k: k == 9, kind_of=lambda b: 2, edit_of=_by_length), 15),
    "letters": lambda: build(make_spec(np.random.default_rng(16), {5: (30, 7), 9: (30, 8)}, [9], leave2=lambda b, k: k == 1, kind_of=lambda b: 2, edit_of=_letters), 16),
    "second_level": lambda: build(make_spec(np.random.default_rng(17), {5: (30, 3), 9: (30, 3)}, [5], kind_of=lambda b: 0, edit_of=_second_level), 17),
    "no_update": lambda: _small(18, upd=[], dead=(55,)),
}
SMALL = ("no_orphan", "first_only", "second_only", "both_in_one_block", "block_loses_every_member", "reverse_orphan", "empty_orphan", "id_ranges", "singleton_first", "two_nodes_of_one_path",
         "dead_entries", "no_update")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def random_case(seed):
    rng = np.random.default_rng(500 + seed)
    ids = sorted(int(x) for x in set(rng.integers(1, 1 << 62, int(rng.integers(2, 14))).tolist()))
    layout = {b: (int(rng.integers(1, 40)), int(rng.integers(0, 6))) for b in ids}
    upd = [b for b in ids if rng.random() < 0.5]
    kinds = {b: int(rng.integers(0, 3)) for b in upd}
    l1 = {(b, k): rng.random() < 0.3 for b in upd for k in range(6)}
    l2 = {(b, k): rng.random() < 0.3 for b in upd for k in range(6)}
    dead = [int(x) for x in rng.integers(1, 1 << 62, int(rng.integers(0, 3))) if int(x) not in layout]
    spec = make_spec(rng, layout, upd, leave1=lambda b, k: l1[(b, k)], leave2=lambda b, k: l2[(b, k)], kind_of=lambda b: kinds[b], reverse=lambda b, k: (b + k) % 3 == 0,
                     orphan_ins=lambda b, k: [(0, "ACGTTGCATT"[:(b + k) % 11])] if (b + k) % 4 else [], n_paths=int(rng.integers(1, 5)), dead=dead)
    return build(spec, 100 + seed)


def all_cases():
    return [(n, case(n)) for n in CASES] + [(f"random_{s}", random_case(s)) for s in range(40)]


# ---------------------------------------------------------------- comparisons
FIELDS = ("counts", "subs", "dels", "inss")


def same(got, want):
    """exact in every field -> the name of the first field that differs, or None (n_cons_letters, the tenth total, depends on the flag and is held elsewhere)"""
    if tuple(got["totals"][:9]) != tuple(want["totals"][:9]):
        return "totals"
    for f in ("blocks", "paths", "nodes", "rc_blocks", "who", "origin", "block_map", "kinds", "orphans", "ins_seq"):
        if list(got[f]) != list(want[f]) if f != "ins_seq" else got[f] != want[f]:
            return f
    for f in FIELDS:
        if got[f].dtype != want[f].dtype or got[f].shape != want[f].shape or got[f].tobytes() != want[f].tobytes():
            return f
    return None


# ---------------------------------------------------------------- the call restated with loops over the tables
def flat_close(t, flags=0):
    """pga_close_round on the tables of close.Tables restated with Python loops after the header's text: the member chain followed through
    the two member_maps, the blocks after merged by id, every list copied from where the chain says -> what CloseOut.to_lists() gives"""
    from pangraph_amd.assemble import _records
    blocks, paths, nodes = t["blocks"], t["paths"], t["nodes"]
    counts = np.asarray(t["counts"], np.int64).reshape(-1, 3)
    src = {0: (_records(t["subs"], SUB), _records(t["dels"], DEL), _records(t["inss"], INS), bytes(t["ins_seq"]))}
    first = np.concatenate([[0], np.cumsum([b[2] if b[3] else 0 for b in blocks])]).astype(np.int64)
    off = np.zeros((len(counts) + 1, 3), np.int64)
    off[1:] = np.cumsum(counts, axis=0)
    upd = list(t.get("upd", []))
    fate = {}                                                                    # global member -> ("final", j, f) | ("orphan", k)
    n1 = 0
    orphans = []
    if upd:
        d1, d2, rc = t["detached"], t["redetached"], t["rc"]
        k1, k2, n1 = sum(d1["n_members"]), sum(d2["n_members"]), len(d1["orphans"])
        counts2 = np.asarray(d2["counts"], np.int64).reshape(-1, 3)
        off2 = np.zeros((len(counts2) + 1, 3), np.int64)
        off2[1:] = np.cumsum(counts2, axis=0)
        src[1] = (_records(d2["subs"], SUB), _records(d2["dels"], DEL), _records(d2["inss"], INS), bytes(rc["ins_seq"]))
        orphans = list(d1["orphans"]) + list(d2["orphans"])
        m = 0
        for j, b in enumerate(upd):
            for s in range(blocks[b][2]):
                v1 = d1["member_map"][m]
                if v1 >= k1:
                    fate[first[b] + s] = ("orphan", v1 - k1)
                else:
                    v2 = d2["member_map"][v1]
                    fate[first[b] + s] = ("orphan", n1 + v2 - k2) if v2 >= k2 else ("final", j, v2)
                m += 1
    r2first = np.concatenate([[0], np.cumsum(t["redetached"]["n_members"])]).astype(np.int64) if upd else [0]
    origin_of_final = {v[2]: a for a, v in fate.items() if v[0] == "final"}
    origin_of_orphan = {v[1]: a for a, v in fate.items() if v[0] == "orphan"}
    after = [(b[0], "s" if i not in upd else "u", i) for i, b in enumerate(blocks) if b[3]] + [(o[2], "o", k) for k, o in enumerate(orphans)]
    after.sort(key=lambda x: x[0])
    assert len({x[0] for x in after}) == len(after), "Conflicting key"
    o_blocks, rc_blocks, picked, who, origin, where, block_map, o_orph = [], [], [], [], [], {}, [NONE] * len(blocks), [None] * len(orphans)
    for i, (bid, what, x) in enumerate(after):
        if what == "s":
            o_blocks.append((bid, blocks[x][1], blocks[x][2], 1)); rc_blocks.append((bytes(t["rc_blocks"][x][0]), blocks[x][2]))
            block_map[x] = i
            for s in range(blocks[x][2]):
                a = int(first[x] + s)
                picked.append((0, counts[a], off[a])); origin.append(a); who.append((t["who"][a][0], int(bool(t["who"][a][1])))); where[a] = (i, s, False)
        elif what == "u":
            j = upd.index(x)
            depth = t["redetached"]["n_members"][j]
            kind, cons = t["rc"]["blocks"][j]
            o_blocks.append((bid, len(cons), depth, 1)); rc_blocks.append((bytes(cons) if kind else bytes(t["rc_blocks"][x][0]), depth))
            block_map[x] = i
            for s in range(depth):
                f = int(r2first[j] + s)
                a = int(origin_of_final[f])
                picked.append((1, counts2[f], off2[f])); origin.append(a); who.append((t["who"][a][0], int(bool(t["who"][a][1])))); where[a] = (i, s, False)
        else:
            o = orphans[x]
            a = int(origin_of_orphan[x])
            o_blocks.append((bid, o[3], 1, 1)); rc_blocks.append((bytes(o[5]), 1))
            picked.append((0, np.zeros(3, np.int64), np.zeros(3, np.int64))); origin.append(a); who.append((t["who"][a][0], 0)); where[a] = (i, 0, True)
            o_orph[x] = (a, o[1], o[2], i, o[3], o[4])
    o_nodes = []
    for nid, p0, p1, b, mem, rev in nodes:
        i, s, orphan = where[int(first[b] + mem)]
        o_nodes.append((nid, p0, p1, i, s, 0 if orphan else int(bool(rev))))
    parts = [[src[w][q][int(o[q]):int(o[q]) + int(n[q])] for w, n, o in picked] for q in range(3)]
    cat = lambda q, dt: np.concatenate(parts[q]) if parts[q] else np.zeros(0, dt)
    subs, dels, inss = cat(0, SUB), cat(1, DEL), cat(2, INS).copy()
    seq, j = bytearray(), 0
    for (w, _, _), e in zip(picked, parts[2]):
        for x in e:
            inss["seq_off"][j] = len(seq)
            seq += src[w][3][int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])]
            j += 1
    out_counts = np.array([p[1] for p in picked], np.uint32).reshape(-1, 3)
    return {"blocks": o_blocks, "paths": [tuple(p) for p in paths], "nodes": o_nodes, "rc_blocks": rc_blocks, "counts": out_counts, "subs": subs, "dels": dels, "inss": inss,
            "ins_seq": bytes(seq), "who": who, "origin": origin, "block_map": block_map, "kinds": [k for k, _ in t["rc"]["blocks"]] if upd else [], "orphans": o_orph,
            "totals": (len(o_blocks), len(paths), len(nodes), len(picked), len(orphans), len(subs), len(dels), len(inss), len(seq))}


# ---------------------------------------------------------------- a case as a flat file for tests/emu/close_emu.cpp
def dump(k, path):
    """the tables of the call in the C layouts (close.Tables), then the expectation: every array as a u64 byte count and its bytes, in the
    order close_emu.cpp's load() reads them (a block record with a pointer goes as the pair cons_len, n_members)"""
    import ctypes as C

    from pangraph_amd import close as cl
    from pangraph_amd.topology import pack_lists
    t, e = k["t"], k["exp"]
    K = cl.Tables(t)
    raw = lambda arr, n: bytes(arr)[:n * C.sizeof(arr._type_)]
    pairs = lambda rows: np.array(rows, np.uint32).reshape(-1, 2).tobytes()
    nb, B, n_paths, P, nn, N = K.graph
    blobs = [raw(B, nb), raw(P, n_paths), raw(N, nn), pairs([(len(c), n) for c, n in t["rc_blocks"]]), K.M.tobytes(), K.S.tobytes(), K.D.tobytes(), K.I.tobytes(), K.L,
             K.W.tobytes(), np.asarray(K.upd, np.uint32).tobytes()]
    if K.d1 is not None:
        for d in (K.d1, K.d2):
            blobs += [pairs([(d.B[i].cons_len, d.B[i].n_members) for i in range(d.out.n_blocks)]), d.map.tobytes(), d.O.tobytes()]
        blobs += [raw(K.RB, len(t["rc"]["blocks"])), raw(K.RM, len(t["rc"]["status"])), K.RL, K.d2.M.tobytes(), K.d2.S.tobytes(), K.d2.D.tobytes(), K.d2.I.tobytes()]
    else:
        blobs += [b""] * 13
    _, EB, _, _, en, EN = pack_lists(e["blocks"], e["paths"], e["nodes"])
    blobs += [raw(EB, len(e["blocks"])), raw(EN, en), e["counts"].tobytes(), e["subs"].tobytes(), e["dels"].tobytes(), e["inss"].tobytes(), e["ins_seq"],
              np.asarray(e["origin"], np.int64).tobytes(), np.asarray(e["block_map"], np.uint32).tobytes()]
    with open(path, "wb") as f:
        for b in blobs:
            f.write(len(b).to_bytes(8, "little") + bytes(b))
