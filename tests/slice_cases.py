"""Inputs for the slicing tests (tests/test_slice_cpu.py, tests/test_gpu_slice.py): the reference's vectors as blocks, random blocks, and the
comparison of what pangraph_amd.slice.slice_blocks returns with the restatement tests/slice_ref.py.  A block here is
{"consensus", "members": [edit], "nodes": [(pos_start, pos_end, path_len, reverse, circular)], "intervals": [slice_ref.interval(...)]}."""
import numpy as np

import slice_ref as sr


def E(inss=(), dels=(), subs=()):
    return {"inss": list(inss), "dels": list(dels), "subs": list(subs)}


def edit_from_json(e):
    return {k: [tuple(x) for x in e[k]] for k in ("subs", "dels", "inss")}


def for_product(blocks):
    """the same blocks as pangraph_amd.slice.slice_blocks takes them: intervals as (start, end, flip)"""
    return [dict(b, intervals=[(i["start"], i["end"], sr.flip_of(i)) for i in b["intervals"]]) for b in blocks]


def expected(blocks):
    """the restatement's answer in the shape of the product's: the offsets are running sums in (block, interval, kept member) order"""
    out = sr.slice_blocks(blocks)
    k = s = d = i = 0
    for rows in out:
        for r in rows:
            r["member_off"] = k
            for v in r["kept"]:
                v["sub_off"], v["del_off"], v["ins_off"] = s, d, i
                s += len(v["subs"]); d += len(v["dels"]); i += len(v["inss"])
                k += 1
    return out


def assert_same(got, exp):
    assert len(got) == len(exp)
    for b, (g_rows, e_rows) in enumerate(zip(got, exp)):
        assert len(g_rows) == len(e_rows), b
        for j, (g, e) in enumerate(zip(g_rows, e_rows)):
            assert g["member_off"] == e["member_off"] and g["dropped"] == e["dropped"], (b, j, g["dropped"][:8], e["dropped"][:8])
            assert len(g["kept"]) == len(e["kept"]), (b, j)
            for a, x in zip(g["kept"], e["kept"]):
                assert a == x, (b, j, x["member"], {k: (a[k], x[k]) for k in x if a[k] != x[k]})


def vector_blocks(V):
    """the reference's unit-test inputs as blocks (nodes where the reference's test has none: a forward node on a linear path)"""
    ex = V["example"]
    blocks = [dict(consensus=ex["consensus"], members=[edit_from_json(ex["edit"])], nodes=[(1000, 1100, 5000, False, False)],
                   intervals=[sr.interval(s["start"], s["end"]) for s in ex["slices"]])]
    nc = V["node_coords"]
    blocks.append(dict(consensus="ACGT" * (nc["block_len"] // 4), members=[edit_from_json(nc["edit"])], nodes=[(0, 200, 5000, False, False)],
                       intervals=[sr.interval(nc["start"], nc["end"])]))
    bs = V["block_slice"]
    nodes = [(n["position"][0], n["position"][1], n["path_len"], n["reverse"], n["circular"]) for n in bs["nodes"]]
    for c in bs["cases"]:
        blocks.append(dict(consensus=bs["consensus"], members=[edit_from_json(e) for e in bs["members"]], nodes=nodes,
                           intervals=[sr.interval(c["start"], c["end"], c["aligned"], c["is_anchor"], c["reverse"])]))
    # the position cases: a member without edits has node_coords == the interval
    for c in V["new_position_circular"] + V["new_position_non_circular"]:
        s, e = c["node_coords"]
        blocks.append(dict(consensus="A" * max(e, 1), members=[E()], nodes=[(c["old_position"][0], c["old_position"][1], c.get("path_len", 0), c["reverse"], "path_len" in c)],
                           intervals=[sr.interval(s, e)]))
    return blocks


def random_seq(rng, n):
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, n)])


def random_intervals(rng, L, n_int, gaps=False):
    """n_int intervals that tile [0, L) (gaps: about a quarter of them taken out again), with random aligned / is_anchor / orientation"""
    cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, L), n_int - 1, replace=False)) + [L]
    ivs = [sr.interval(a, b, bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for a, b in zip(cuts, cuts[1:])]
    if gaps and len(ivs) > 1:
        keep = rng.random(len(ivs)) > 0.25
        keep[int(rng.integers(0, len(ivs)))] = True
        ivs = [i for i, k in zip(ivs, keep) if k]
    return ivs


def random_member(rng, L, n_subs, n_dels, n_inss, edges=(), shuffled=False, long_dels=False):
    """an edit whose deletions do not overlap one another (zero-length ones aside) and whose insertions lie outside the deletions or at
    their ends; `edges`: positions (interval boundaries) the edits are drawn to"""
    edges = [p for p in edges if 0 <= p <= L]
    pts = sorted(int(x) for x in rng.choice(np.arange(0, L + 1), 2 * n_dels, replace=False)) if n_dels else []
    if long_dels:                                                          # fewer, longer deletions: pair the sorted points the other way round
        dels = [(a, b - a) for a, b in zip(pts[0::2], pts[1::2])]
    else:                                                                  # short ones: at most a few letters each
        dels = [(a, min(b - a, int(rng.integers(1, 6)))) for a, b in zip(pts[0::2], pts[1::2])]
    dels = [(a, 0) if rng.random() < 0.1 else (a, n) for a, n in dels]     # some of length 0, inside an interval or on a boundary
    deleted = np.zeros(L + 1, dtype=bool)
    for a, n in dels:
        deleted[a + 1:a + n] = True                                        # the inside of a deletion: no insertion there
    free = np.flatnonzero(~deleted)

    def draw(n, top):
        out = []
        for _ in range(n):
            p = int(edges[int(rng.integers(0, len(edges)))]) + int(rng.integers(-1, 2)) if edges and rng.random() < 0.3 else int(rng.integers(0, top))
            out.append(min(max(p, 0), top - 1))
        return out
    subs = [(p, "ACGT"[int(rng.integers(0, 4))]) for p in sorted(draw(n_subs, L))]
    ins_pos = [int(free[np.searchsorted(free, p)]) if p <= free[-1] else int(free[-1]) for p in sorted(draw(n_inss, L + 1))]
    inss = [(p, random_seq(rng, int(rng.integers(1, 6)))) for p in sorted(ins_pos)]
    if shuffled:
        subs, dels, inss = ([lst[k] for k in rng.permutation(len(lst))] for lst in (subs, dels, inss))
    return E(inss, dels, subs)


def random_node(rng, room):
    """an old node with room for `room` letters: linear or circular, forward or reverse, some circular ones wrapping"""
    circular, reverse = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    if circular:
        path_len = room + int(rng.integers(0, 3 * room + 1))
        start = int(rng.integers(0, path_len))
        return (start, (start + room) % path_len, path_len, reverse, True)
    start = int(rng.integers(0, 10 ** 6))
    return (start, start + room, start + room + int(rng.integers(0, 1000)), reverse, False)


def room_of(L, e):
    return L + sum(len(s) for _, s in e["inss"])


def random_block(rng, L, n_members, list_len, n_int, shuffled=False, gaps=False, specials=True):
    """a block of n_members members with list_len substitutions, deletions and insertions each, cut into n_int intervals.  With `specials`
    (blocks of eight members and more) the first members are made to hit what the random ones may miss: an insertion at the end of the block, a member that one long deletion
    removes from several slices, and two overlapping deletions whose lengths add up to a slice without covering it."""
    cons = random_seq(rng, L)
    ivs = random_intervals(rng, L, n_int, gaps)
    edges = sorted(set([i["start"] for i in ivs] + [i["end"] for i in ivs]))
    members = []
    for m in range(n_members):
        members.append(random_member(rng, L, list_len, list_len, list_len, edges, shuffled, long_dels=(m % 4 == 3)))
    if specials and n_members >= 8:
        wide = next((i for i in ivs if i["end"] - i["start"] >= 4 and i["start"] >= 1), None)
        sp = [E(inss=[(L, "ACG"), (0, "T")], subs=[(L - 1, "A")]), E(dels=[(0, L)]), E(dels=[(ivs[0]["start"], ivs[-1]["end"] - ivs[0]["start"])], inss=[(L, "GG")])]
        if wide is not None:                                               # lengths n - 1 and 1 + ... : sum == the slice, last letter left
            s, n = wide["start"], wide["end"] - wide["start"]
            sp.append(E(dels=[(s, n - 2), (s + 1, 2)] if not shuffled else [(s + 1, 2), (s, n - 2)]))
        for k, e in enumerate(sp):
            members[k] = e
    nodes = [random_node(rng, room_of(L, e)) for e in members]
    return dict(consensus=cons, members=members, nodes=nodes, intervals=ivs)
