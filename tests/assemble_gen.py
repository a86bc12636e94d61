"""Inputs for pga_assemble_blocks (pangraph_amd/assemble.py) and the expectation they are held against.  A case stands on a case of
tests/apply_gen.py: its cut, slices and `exp` -- what pga_apply_merge returns, computed from the host reweave() of pangraph_amd/reweave.py --
are the tables of the call; its dict graph `after` (the merged block = the anchor half united with the append half) says who sits where.
The edit lists are data to this entry, so they are made here, seeded: one for every member of the graph before (the cut blocks' too: they lie
between the survivors' lists), one for every kept slice member, one result for every member of an append slice.  Insertion letters point
into two pools at random places: shared, shuffled and overlapping seq_off come with that; one insertion of each pool ends exactly at its end.

`host_assemble` flattens the dict graph after in ascending block id, within a block in ascending node id, and looks every node's edit up by
what the node is -- it never reads member_src.  A case is {"t": the tables of assemble.Tables, "exp": {flags: what assemble_blocks returns},
"c": the apply_gen case, "k_append": the slice members whose edits are promise results}."""
import functools

import numpy as np

import apply_gen as ag
import topo_gen as tg
from pangraph_amd.assemble import MERGED_ONLY, TILE
from pangraph_amd.detach import DEL, INS, SUB

NONE = ag.NONE
LENGTHS = (0, 0, 0, 1, 2, 63, 64, 65, 130)
INS_LETTERS = (0, 1, 63, 64, 65, 127, 128, 5000)
POOL = 6000                                # letters per pool


def _edit(rng, n_subs, n_dels, n_inss, ins_lens=None):
    """-> (subs, dels, inss) records; an insertion's letters lie anywhere in its pool"""
    s, d, i = np.zeros(n_subs, SUB), np.zeros(n_dels, DEL), np.zeros(n_inss, INS)
    s["pos"], s["alt"] = rng.integers(0, 1 << 20, n_subs), rng.choice(np.frombuffer(b"ACGTN", np.uint8), n_subs)
    d["pos"], d["len"] = rng.integers(0, 1 << 20, n_dels), rng.integers(0, 50, n_dels)
    i["pos"] = rng.integers(0, 1 << 20, n_inss)
    i["len"] = ins_lens if ins_lens is not None else np.where(rng.random(n_inss) < 0.2, 0, rng.integers(0, 41, n_inss))
    i["seq_off"] = (rng.random(n_inss) * (POOL - i["len"] + 1)).astype(np.uint64)
    return s, d, i


def random_edit(rng):
    return _edit(rng, *(LENGTHS[k] for k in rng.integers(0, len(LENGTHS), 3)))


EMPTY = (np.zeros(0, SUB), np.zeros(0, DEL), np.zeros(0, INS))


def _flat(edits):
    """edits in order -> (counts, subs, dels, inss)"""
    counts = np.array([[len(e[0]), len(e[1]), len(e[2])] for e in edits], np.uint32).reshape(-1, 3)
    cat = lambda k, dt: np.concatenate([e[k] for e in edits]) if edits else np.zeros(0, dt)
    return counts, cat(0, SUB), cat(1, DEL), cat(2, INS)


def _offsets(counts):
    c = counts.astype(np.int64)
    return np.cumsum(c, axis=0) - c


def host_assemble(c, before_edit, slice_edit, result_edit, pools):
    """c: an apply_gen case; before_edit[node id], slice_edit[k], result_edit[k] (k of an append slice): (subs, dels, inss); pools: the two
    letter buffers -> {0: the default mode's arrays, MERGED_ONLY: the merged blocks'} as assemble.AssembleOut.to_arrays() gives them"""
    blocks, _, _, cut, ivs, slices, _ = c["args"]
    before, after, exp = c["before"], c["after"], c["exp"]
    member_before, m = {}, 0
    for bid, _, _, alive in blocks:
        for nid in (sorted(before["blocks"][bid]["alignments"]) if alive else []):
            member_before[nid] = m
            m += 1
    k_of = {n[0]: k for k, n in enumerate(exp["new_nodes"])}
    append = {k for s, iv in enumerate(ivs) if iv["aligned"] and not iv["is_anchor"] for k in range(slices[s][0], slices[s][0] + slices[s][1])}
    merged = {iv["new_block_id"] for iv in ivs if iv["aligned"]}
    res = {}
    for flags in (0, MERGED_ONLY):
        out_blocks, edits, src, who, origin = [], [], [], [], []
        for bid in sorted(after["blocks"]):
            if flags and bid not in merged:
                continue
            blk = after["blocks"][bid]
            out_blocks.append((blk["consensus"].encode(), len(blk["alignments"])))
            for nid in sorted(blk["alignments"]):
                if nid in k_of:
                    k = k_of[nid]
                    edits.append(result_edit[k] if k in append else slice_edit[k]); src.append(1 if k in append else 0); origin.append(-(1 + k))
                else:
                    edits.append(before_edit[nid]); src.append(0); origin.append(member_before[nid])
                who.append((nid, int(after["nodes"][nid]["strand"] == "-")))
        counts, subs, dels, inss = _flat(edits)
        letters = bytearray()
        inss = inss.copy()
        at = 0
        for e, p in zip(edits, src):
            for x in e[2]:
                letters += pools[p][int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])]
                inss["seq_off"][at] = len(letters) - int(x["len"])
                at += 1
        res[flags] = {"blocks": out_blocks, "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": bytes(letters), "who": who if cut else None,
                      "origin": origin, "totals": (len(out_blocks), len(edits), len(subs), len(dels), len(inss), len(letters))}
    return res, append


def build(c, seed=0, before=None, sliced=None, result=None, pool0=None):
    """c: an apply_gen case; before / sliced / result: (rng, running index: the member before, the slice member, the rank among the append members) ->
    an edit, default random_edit; pool0: the caller's letter buffer (at least POOL letters; the edits of `before` point into it and stay
    as they are) -> the case"""
    rng = np.random.default_rng(9000 + seed)
    pools = [bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), POOL)) for _ in range(2)]
    if pool0 is not None:
        assert len(pool0) >= POOL
        pools[0] = bytes(pool0)
    blocks, _, _, cut, ivs, slices, members = c["args"]
    exp = c["exp"]
    pick = lambda f, idx: f(rng, idx) if f else random_edit(rng)
    before_edit, order = {}, []
    for bid, _, _, alive in blocks:
        for nid in (sorted(c["before"]["blocks"][bid]["alignments"]) if alive else []):
            before_edit[nid] = pick(before, len(order))
            order.append(nid)
    append = {k for s, iv in enumerate(ivs) if iv["aligned"] and not iv["is_anchor"] for k in range(slices[s][0], slices[s][0] + slices[s][1])}
    slice_edit = [pick(sliced, k) for k in range(len(members))]
    result_edit = {k: pick(result, r) for r, k in enumerate(sorted(append))}
    used = [e for k, e in enumerate(slice_edit) if k not in append] + (list(before_edit.values()) if pool0 is None else [])
    used_ins = [e[2] for e in used if e[2]["len"].any()]
    for some in (used_ins, [e[2] for e in result_edit.values() if e[2]["len"].any()]):
        if some:                                                             # one insertion with letters ends exactly at the end of its buffer
            at = int(np.flatnonzero(some[0]["len"])[0])
            some[0]["seq_off"][at] = (POOL if some is not used_ins or pool0 is None else len(pool0)) - int(some[0]["len"][at])
    want, append2 = host_assemble(c, before_edit, slice_edit, result_edit, pools)
    assert append2 == append
    counts, subs, dels, inss = _flat([before_edit[n] for n in order])
    s_counts, s_subs, s_dels, s_inss = _flat(slice_edit)
    s_off = _offsets(s_counts)
    at = {b[0]: i for i, b in enumerate(blocks) if b[3]}
    interval_of = {(iv["new_block_id"], bool(iv["is_anchor"])): s for s, iv in enumerate(ivs) if iv["aligned"]}
    promises = [(interval_of[(q["new_block_id"], True)], interval_of[(q["new_block_id"], False)]) for q in c["promises"]]
    rows = [k for _, q in promises for k in range(slices[q][0], slices[q][0] + slices[q][1])]
    r_counts, p_subs, p_dels, p_inss = _flat([result_edit[k] for k in rows])
    r_off = _offsets(r_counts)
    t = {"blocks": [(c["before"]["blocks"][b[0]]["consensus"].encode(), b[2]) if b[3] else (b"", 0) for b in blocks],
         "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": pools[0],
         "cut": list(cut), "intervals": list(ivs), "promises": promises, "slices": list(slices),
         "s_members": np.concatenate([s_counts.astype(np.uint64), s_off.astype(np.uint64)], axis=1) if len(members) else [],
         "s_subs": s_subs, "s_dels": s_dels, "s_inss": s_inss,
         "res": np.concatenate([np.zeros((len(rows), 1), np.int64), r_counts.astype(np.int64), r_off], axis=1) if rows else [],
         "p_subs": p_subs, "p_dels": p_dels, "p_inss": p_inss, "p_ins_seq": pools[1],
         "applied": {k: exp[k] for k in ("blocks", "nodes", "new_blocks", "member_src", "block_map")} if cut else None}
    return {"t": t, "exp": want, "c": c, "k_append": append, "rows": rows, "at": at, "node_order": order, "pools": pools}


# ---------------------------------------------------------------- the named cases
A_LEN = {"A": 30, "B": 25, "C": 5}
MERGE_PATHS = [(False, "A+ B+"), (False, "B- A-"), (True, "A+ C+ B+"), (True, "B+ A-")]
MERGE_CUT = {1: [(0, 20, 900, True, True), (20, 30, 901, False, False)], 2: [(0, 5, 902, False, False), (5, 25, 900, True, False)]}


def _merge(drop):
    return ag.synth(tg.graph(MERGE_PATHS, lens=A_LEN), MERGE_CUT, drop=drop)


def _single_deletion(rng, k):
    """what solve_promise gives a member whose sequence is empty: the one deletion (0, anchor_len) (anchor_len: 20 in MERGE_CUT)"""
    return (np.zeros(0, SUB), np.array([(0, 20)], DEL), np.zeros(0, INS))


def _members_graph(n_a, n_b):
    """block A with n_a members, block B with n_b, block X cut into 5 pieces: the members after are n_a + n_b + 5"""
    return ag.synth(tg.graph([(False, " ".join(["A+"] * n_a + ["B+"] * n_b + ["X+"]))], lens={"A": 4, "B": 6, "X": 50}), {3: ag.pieces(5, 10, 7000)})


def _one_heavy(rng, idx):
    return _edit(rng, 5000, 0, 3000) if idx == 700 else EMPTY


def _by_length(rng, idx):
    return _edit(rng, idx % 131, (idx + 50) % 131, (idx + 100) % 131)


def _letters(rng, idx):
    return _edit(rng, 1, 0, len(INS_LETTERS), ins_lens=np.array(INS_LETTERS)) if idx % 3 == 0 else random_edit(rng)


def _second_level(rng, idx):
    return _edit(rng, TILE * TILE + 1, 3, 2) if idx == 1 else _edit(rng, 2, 1, 1)


CASES = {
    "reference": lambda: build(ag.case("reference")),
    "alternating": lambda: build(ag.case("interleaved_merge"), 1),
    "only_append": lambda: build(_merge(lambda b, m, j: b == 1 and j == 0), 2),
    "only_anchor": lambda: build(_merge(lambda b, m, j: b == 2 and j == 1), 3),
    "empty_unaligned": lambda: build(ag.case("empty_unaligned"), 4),
    "single_deletion": lambda: build(ag.case("interleaved_merge"), 5, result=_single_deletion),
    "no_cut": lambda: build(ag.case("no_cut"), 6),
    "id_ranges": lambda: build(ag.case("id_ranges"), 7),
    "high_index": lambda: build(ag.case("high_index"), 8),
    "members_1023": lambda: build(_members_graph(1000, 18), 9, before=lambda rng, i: _edit(rng, i % 3, i % 2, (i + 1) % 2)),
    "members_1024": lambda: build(_members_graph(1000, 19), 10, before=lambda rng, i: _edit(rng, i % 3, i % 2, (i + 1) % 2)),
    "members_1025": lambda: build(_members_graph(1000, 20), 11, before=lambda rng, i: _edit(rng, i % 3, i % 2, (i + 1) % 2)),
    "straddle": lambda: build(_members_graph(1000, 100), 12, before=lambda rng, i: _edit(rng, i % 3, i % 2, (i + 1) % 2)),
    "one_heavy": lambda: build(_members_graph(1500, 501), 13, before=_one_heavy, sliced=lambda rng, k: EMPTY),
    "list_lengths": lambda: build(_members_graph(200, 100), 14, before=_by_length, sliced=_by_length),
    "letters": lambda: build(ag.case("interleaved_merge"), 15, before=_letters, sliced=_letters, result=_letters),
    "second_level": lambda: build(ag.case("interleaved_merge"), 16, result=_second_level, sliced=lambda rng, k: _edit(rng, 2, 1, 1)),
}
SMALL = ("reference", "alternating", "only_append", "only_anchor", "empty_unaligned", "single_deletion", "id_ranges", "letters")


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def random_case(seed):
    return build(ag.random_case(seed), 100 + seed)


def all_cases():
    return [(n, case(n)) for n in CASES] + [(f"random_{s}", random_case(s)) for s in range(40)]


# ---------------------------------------------------------------- comparisons
FIELDS = ("counts", "subs", "dels", "inss")


def same(got, want):
    """exact in every field -> the name of the first field that differs, or None"""
    for f in ("totals", "blocks", "who", "origin", "ins_seq"):
        if got[f] != want[f]:
            return f
    for f in FIELDS:
        if got[f].dtype != want[f].dtype or got[f].shape != want[f].shape or got[f].tobytes() != want[f].tobytes():
            return f
    return None


def resolved(a, letters=None):
    """the insertions of an arrays dict with their letters looked up: [(pos, letters)]"""
    letters = a["ins_seq"] if letters is None else letters
    return [(int(x["pos"]), bytes(letters[int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])])) for x in a["inss"]]


def merged_blocks_input(k):
    """the case as detach.merged_blocks takes it: (anchor, append), the anchor halves packed from the sliced lists, the append halves from the results"""
    t, c = k["t"], k["c"]
    slices, sm = t["slices"], np.asarray(t["s_members"], np.int64).reshape(-1, 6)
    ids = [n[0] for n in c["exp"]["new_nodes"]]
    anchor_k = [x for a, _ in t["promises"] for x in range(slices[a][0], slices[a][0] + slices[a][1])]
    gather = lambda src, col: np.concatenate([src[sm[x, 3 + col]:sm[x, 3 + col] + sm[x, col]] for x in anchor_k]) if anchor_k else src[:0]
    anchor = {"cons": [t["blocks"][t["cut"][_cut_of(t, a)][0]][0][t["intervals"][a]["start"]:t["intervals"][a]["end"]] for a, _ in t["promises"]],
              "n_members": [slices[a][1] for a, _ in t["promises"]], "node_ids": [ids[x] for x in anchor_k], "counts": sm[anchor_k, :3] if anchor_k else np.zeros((0, 3)),
              "subs": gather(t["s_subs"], 0), "dels": gather(t["s_dels"], 1), "inss": gather(t["s_inss"], 2), "ins_seq": t["ins_seq"]}
    res = np.asarray(t["res"], np.int64).reshape(-1, 7)
    append = {"n_members": [slices[q][1] for _, q in t["promises"]], "node_ids": [ids[x] for x in k["rows"]], "res": res[:, 1:],
              "subs": t["p_subs"], "dels": t["p_dels"], "inss": t["p_inss"], "ins_seq": t["p_ins_seq"]}
    return anchor, append


def _cut_of(t, interval):
    return [i for i, cb in enumerate(t["cut"]) if cb[2] <= interval < cb[2] + cb[1]][0]


def dicts_of(a):
    """an arrays dict -> per block {"consensus", "members": [edit]} as reconstruct._Packed takes them"""
    res, m, off, ins = [], 0, [0, 0, 0], resolved(a)
    for cons, n in a["blocks"]:
        members = []
        for _ in range(n):
            c = [int(x) for x in a["counts"][m]]
            members.append({"subs": [(int(x["pos"]), chr(int(x["alt"]))) for x in a["subs"][off[0]:off[0] + c[0]]],
                            "dels": [(int(x["pos"]), int(x["len"])) for x in a["dels"][off[1]:off[1] + c[1]]],
                            "inss": [(p, s.decode()) for p, s in ins[off[2]:off[2] + c[2]]]})
            off = [off[q] + c[q] for q in range(3)]
            m += 1
        res.append({"consensus": cons.decode(), "members": members})
    return res


def list_assemble(t, flags=0):
    """pga_assemble_blocks on the tables of assemble.Tables restated with Python loops after the header's text: the block table after walked
    in order, member_src followed slot by slot -> what AssembleOut.to_arrays() gives.  Stands in for the call where there is no device."""
    from pangraph_amd.assemble import _records
    rec = lambda name, dt: _records(t.get(name, []), dt)
    lists = {0: (rec("subs", SUB), rec("dels", DEL), rec("inss", INS)), 1: (rec("s_subs", SUB), rec("s_dels", DEL), rec("s_inss", INS)), 2: (rec("p_subs", SUB), rec("p_dels", DEL), rec("p_inss", INS))}
    letters = {0: bytes(t["ins_seq"]), 1: bytes(t["ins_seq"]), 2: bytes(t.get("p_ins_seq", b""))}
    counts = np.asarray(t["counts"], np.int64).reshape(-1, 3)
    first, before_off = np.concatenate([[0], np.cumsum([n for _, n in t["blocks"]])]), _offsets(counts) if len(counts) else counts
    picked = []                                                                  # per output member: (source, counts, offsets, origin)
    out_blocks, who = [], []
    cut, ap = t.get("cut", []), t.get("applied")
    if not cut:
        for b, (cons, n) in enumerate(t["blocks"] if not flags else []):
            out_blocks.append((bytes(cons), n))
            picked += [(0, counts[m], before_off[m], int(m)) for m in range(first[b], first[b + 1])]
    else:
        ivs, slices, sm, res = t["intervals"], t["slices"], np.asarray(t["s_members"], np.int64).reshape(-1, 6), np.asarray(t["res"], np.int64).reshape(-1, 7)
        block_of = {s: blk for blk, n, f in cut for s in range(f, f + n)}
        first_res, at = {}, 0
        for a, q in t["promises"]:
            first_res[q] = at
            at += slices[q][1]
        made = {e[0]: e for e in ap["new_blocks"]}
        old_of = {new: old for old, new in enumerate(ap["block_map"]) if new != NONE}
        node_at = {(n[3], n[4]): (n[0], int(n[5])) for n in ap["nodes"]}
        for i, blk in enumerate(ap["blocks"]):
            if flags and not (i in made and made[i][1] == 1):
                continue
            if i in old_of:
                b = old_of[i]
                out_blocks.append((bytes(t["blocks"][b][0]), t["blocks"][b][1]))
                picked += [(0, counts[m], before_off[m], int(m)) for m in range(first[b], first[b + 1])]
            else:
                _, kind, ia, ib, member_off = made[i]
                out_blocks.append((bytes(t["blocks"][block_of[ia]][0])[ivs[ia]["start"]:ivs[ia]["end"]], blk[2]))
                for s in range(blk[2]):
                    k = int(ap["member_src"][member_off + s])
                    if kind == 1 and slices[ib][0] <= k < slices[ib][0] + slices[ib][1]:
                        r = res[first_res[ib] + k - slices[ib][0]]
                        assert r[0] == 0
                        picked.append((2, r[1:4], r[4:7], -(1 + k)))
                    else:
                        assert slices[ia][0] <= k < slices[ia][0] + slices[ia][1]
                        picked.append((1, sm[k, :3], sm[k, 3:], -(1 + k)))
            who += [node_at[(i, s)] for s in range(blk[2])]
    edits = [tuple(lists[src][q][int(off[q]):int(off[q]) + int(n[q])] for q in range(3)) for src, n, off, _ in picked]
    out_counts, subs, dels, inss = _flat(edits)
    inss, seq = inss.copy(), bytearray()
    j = 0
    for (src, _, _, _), e in zip(picked, edits):
        for x in e[2]:
            inss["seq_off"][j] = len(seq)
            seq += letters[src][int(x["seq_off"]):int(x["seq_off"]) + int(x["len"])]
            j += 1
    return {"blocks": out_blocks, "counts": out_counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": bytes(seq), "who": who if cut else None,
            "origin": [o for _, _, _, o in picked], "totals": (len(out_blocks), len(picked), len(subs), len(dels), len(inss), len(seq))}
