"""Measurement only (not a test): pga_close_round on the largest generated cases of tests/close_gen.py and on a synthetic round in the
proportions of a merged level of levels.py's 16-genome population, beside the dict route a host without the entry takes for the same tail
(detach.detach_graph, the block replacement, detach_graph on the kind-2 blocks, then the flat arrays rebuilt from the dicts).
levels.py yields genomes and find_matches batches, not block arrays (the assemble section), so the level is made here.
Run on an MI355X:  python dev/close_bench.py"""
import copy
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import close_gen as cg  # noqa: E402
from pangraph_amd import batch, close as cl, detach as dt  # noqa: E402
from pangraph_amd.detach import DEL, INS, SUB  # noqa: E402
from pangraph_amd.reconstruct import _Packed  # noqa: E402
from pangraph_amd.topology import pack_lists  # noqa: E402


def device(t, label, check=None):
    dll = batch.lib()
    K = cl.Tables(t)
    cl.close_round_raw(*K.call_args(), dll=dll, keep=K).free()                    # warm-up
    for flags in (0, cl.COPY_CONSENSUS):
        t0 = time.perf_counter()
        out = cl.close_round_raw(*K.call_args(), flags=flags, dll=dll, keep=K)
        wall = (time.perf_counter() - t0) * 1e3
        ms = cl.last_ms(dll)
        o = out.out
        print(f"{label} flags={flags}: call {wall:.2f} ms (uploads {ms[0]:.2f}, kernels {ms[1]:.2f}, downloads {ms[2]:.2f}); after: {o.n_blocks} blocks, {o.n_members} members, "
              f"{o.n_orphans} orphans, {o.n_subs} subs, {o.n_inss} inss, {o.n_ins_letters} letters, {o.n_cons_letters} consensus bytes owned")
        if check is not None and flags == 0:
            got = out.to_lists()
            print(f"{label}: against the restatement in loops: {cg.same(got, check) or 'same'}")
        out.free()


def dict_route(k, label):
    """the same tail on dicts with the device's detach, then the two flat layouts packed again from the dicts"""
    spec = k["spec"]
    g = copy.deepcopy({f: spec[f] for f in ("blocks", "nodes", "paths")})
    dll = batch.lib()
    dt.detach_graph(copy.deepcopy(g), spec["upd"], dll=dll)                       # warm-up
    t0 = time.perf_counter()
    dt.detach_graph(g, spec["upd"], dll=dll)
    for b in spec["upd"]:
        kind, cons, edits = spec["rc"][b]
        g["blocks"][b] = {"consensus": cons, "alignments": {n: e for n, e in edits.items()}}
    dt.detach_graph(g, [b for b in spec["upd"] if spec["rc"][b][0] == 2], dll=dll)
    t1 = time.perf_counter()
    blocks, paths, nodes, order = cg.graph_lists(g)
    pack_lists(blocks, paths, nodes)
    _Packed([{"consensus": g["blocks"][b[0]]["consensus"], "members": [g["blocks"][b[0]]["alignments"][n] for n in order[b[0]]]} for b in blocks], [])
    t2 = time.perf_counter()
    print(f"{label}: dict route {1e3 * (t2 - t0):.1f} ms (detach_graph x2 and the replacement {1e3 * (t1 - t0):.1f}, the flat arrays again {1e3 * (t2 - t1):.1f})")


def level(n_merged=200, depth=128, n_other=400, other_depth=64, seed=1):
    """a synthetic round: n_merged updated blocks of `depth` members (an anchor and an append block of a 16-genome level joined), n_other
    untouched blocks; a member has about 20 substitutions, 3 deletions and 3 insertions of about 6 letters; one member in a hundred leaves in
    each stage; every updated block was realigned"""
    rng = np.random.default_rng(seed)
    nb = n_merged + n_other
    is_upd = np.zeros(nb, bool)
    is_upd[rng.choice(nb, n_merged, replace=False)] = True
    depths = np.where(is_upd, depth, other_depth)
    blocks = [(1000 * (i + 1), 500, int(depths[i]), 1) for i in range(nb)]
    first = np.concatenate([[0], np.cumsum(depths)])
    nm = int(first[-1])
    who = [(10 + m, int(m % 5 == 0)) for m in range(nm)]
    order = rng.permutation(nm)
    block_of = np.repeat(np.arange(nb), depths)
    n_paths = 16
    per = nm // n_paths
    paths = [(p + 1, p * per, per if p < n_paths - 1 else nm - p * per, 0) for p in range(n_paths)]
    nodes = [(10 + int(m), 7 * i, 7 * i + 500, int(block_of[m]), int(m - first[block_of[m]]), int(m % 5 == 0)) for i, m in enumerate(order)]

    def lists(n, letters):
        counts = np.stack([rng.integers(15, 26, n), rng.integers(2, 5, n), rng.integers(2, 5, n)], axis=1).astype(np.uint32)
        s, d, i = np.zeros(int(counts[:, 0].sum()), SUB), np.zeros(int(counts[:, 1].sum()), DEL), np.zeros(int(counts[:, 2].sum()), INS)
        s["pos"], s["alt"] = rng.integers(0, 500, len(s)), 65
        d["pos"], d["len"] = rng.integers(0, 400, len(d)), rng.integers(0, 5, len(d))
        i["pos"], i["len"] = rng.integers(0, 500, len(i)), rng.integers(3, 10, len(i))
        i["seq_off"] = rng.integers(0, len(letters) - 10, len(i))
        return counts, s, d, i
    pool = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1 << 20))
    pool2 = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 1 << 19))
    counts, subs, dels, inss = lists(nm, pool)
    upd = [int(b) for b in np.flatnonzero(is_upd)]
    merged = [int(first[b] + s) for b in upd for s in range(depth)]
    gone1 = [m % 97 == 5 for m in range(len(merged))]
    k1 = len(merged) - sum(gone1)
    ids = iter(int(x) for x in rng.integers(1, 1 << 63, 4 * len(merged)) if int(x) % 1000)
    map1, o1, kept = [], [], 0
    for m, a in enumerate(merged):
        if gone1[m]:
            map1.append(k1 + len(o1)); o1.append((m, who[a][0], next(ids), 40, 0, pool[m:m + 40]))
        else:
            map1.append(kept); kept += 1
    kept1 = [sum(1 for m in range(j * depth, (j + 1) * depth) if not gone1[m]) for j in range(n_merged)]
    src1 = [m for m in range(len(merged)) if not gone1[m]]
    gone2 = [m1 % 89 == 7 for m1 in range(k1)]
    k2 = k1 - sum(gone2)
    map2, o2, kept = [], [], 0
    for m1 in range(k1):
        if gone2[m1]:
            map2.append(k2 + len(o2)); o2.append((m1, who[merged[src1[m1]]][0], next(ids), 30, 0, pool2[m1:m1 + 30]))
        else:
            map2.append(kept); kept += 1
    at, kept2 = 0, []
    for n in kept1:
        kept2.append(sum(1 for m1 in range(at, at + n) if not gone2[m1])); at += n
    counts2, subs2, dels2, inss2 = lists(k2, pool2)
    cons = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 500))
    return {"blocks": blocks, "paths": paths, "nodes": nodes, "rc_blocks": [(cons, int(d)) for d in depths], "counts": counts, "subs": subs, "dels": dels, "inss": inss,
            "ins_seq": pool, "who": who, "upd": upd,
            "detached": {"n_members": kept1, "member_map": map1, "orphans": o1},
            "rc": {"blocks": [(2, cons[:490] + b"ACGTACGTAC")] * n_merged, "status": [0] * k1, "ins_seq": pool2},
            "redetached": {"n_members": kept2, "member_map": map2, "orphans": o2, "counts": counts2, "subs": subs2, "dels": dels2, "inss": inss2}}


if __name__ == "__main__":
    for name in ("list_lengths", "one_heavy_updated", "high_index", "second_level"):
        k = cg.case(name)
        device(k["t"], name)
        dict_route(k, name)
    t = level()
    device(t, "level of 200 merged blocks x 128 members beside 400 x 64", check=cg.flat_close(t))
    device(level(2000, 128, 4000, 64, seed=2), "level of 2000 merged blocks x 128 members beside 4000 x 64")
