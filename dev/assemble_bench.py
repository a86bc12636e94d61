"""One pga_assemble_blocks call at the size of a merged tree level against detach.merged_blocks() (the numpy gather on the host) on the same
input, once each after a warm-up.  The level is synthetic, in the proportions of a merge of pangraph_amd/levels.py's populations: every
promise joins an anchor block and an append block of --depth members each, beside --survivors blocks that no match touches; a member
carries --subs substitutions, --dels deletions and --inss insertions of --letters letters.
    python dev/assemble_bench.py [--promises 2000 --depth 64 --survivors 4000 --subs 20 --dels 3 --inss 3 --letters 6]
Prints one JSON line: sizes, merged_only_ms / default_ms (the call: uploads, kernels, downloads; wall clock), stream_ms (pga_assemble_last_ms
of the merged-only call), host_ms (merged_blocks, which builds the merged blocks only), same (the two agree)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pangraph_amd import assemble as asm  # noqa: E402
from pangraph_amd import detach as dt  # noqa: E402


def lists(rng, n_members, a, pool):
    """-> (counts (n, 3), subs, dels, inss) for n_members members, about a.subs / a.dels / a.inss entries each"""
    counts = np.stack([rng.poisson(x, n_members) for x in (a.subs, a.dels, a.inss)], axis=1).astype(np.uint32)
    n = counts.sum(axis=0)
    s, d, i = np.zeros(n[0], dt.SUB), np.zeros(n[1], dt.DEL), np.zeros(n[2], dt.INS)
    s["pos"], s["alt"] = rng.integers(0, 1000, n[0]), 65
    d["pos"], d["len"] = rng.integers(0, 1000, n[1]), rng.integers(1, 9, n[1])
    i["pos"], i["len"] = rng.integers(0, 1000, n[2]), rng.poisson(a.letters, n[2])
    i["seq_off"] = rng.integers(0, pool - 64, n[2])
    return counts, s, d, i


def offsets(counts):
    c = counts.astype(np.int64)
    return np.cumsum(c, axis=0) - c


def build(a):
    rng = np.random.default_rng(11)
    P, A, V, pool = a.promises, a.depth, a.survivors, 1 << 20
    letters = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), pool))
    cons = b"A" * 1000
    nb, nk = 2 * P + V, 2 * P * A
    counts, subs, dels, inss = lists(rng, nb * A, a, pool)                        # the graph before: every block has A members
    s_counts, s_subs, s_dels, s_inss = lists(rng, nk, a, pool)                    # the slices: one interval per cut block, every member kept
    r_counts, p_subs, p_dels, p_inss = lists(rng, P * A, a, pool)                 # the results of the append members
    nid = rng.permutation(np.arange(1, nk + V * A + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(1))
    k = np.arange(nk)
    member_src = np.lexsort((nid[:nk], (k // A) % P)).astype(np.uint64)            # merged block p: the members of slices p and P + p by node id
    ivs = [{"new_block_id": 10 * (c % P + 1) + 5, "start": 0, "end": 1000, "aligned": 1, "is_anchor": int(c < P)} for c in range(2 * P)]
    nodes = np.zeros((nk + V * A, 6), np.uint64)
    nodes[:nk, 0], nodes[:nk, 3], nodes[:nk, 4] = nid[member_src.astype(np.int64)], k // (2 * A), k % (2 * A)
    nodes[nk:, 0], nodes[nk:, 3], nodes[nk:, 4] = nid[nk:], P + np.arange(V * A) // A, np.arange(V * A) % A
    nodes[:, 5] = rng.integers(0, 2, len(nodes))
    t = {"blocks": [(cons, A)] * nb, "counts": counts, "subs": subs, "dels": dels, "inss": inss, "ins_seq": letters,
         "cut": [(c, 1, c) for c in range(2 * P)], "intervals": ivs, "promises": [(p, P + p) for p in range(P)], "slices": [(c * A, A, 0) for c in range(2 * P)],
         "s_members": np.concatenate([s_counts.astype(np.uint64), offsets(s_counts).astype(np.uint64)], axis=1), "s_subs": s_subs, "s_dels": s_dels, "s_inss": s_inss,
         "res": np.concatenate([np.zeros((P * A, 1), np.int64), r_counts.astype(np.int64), offsets(r_counts)], axis=1), "p_subs": p_subs, "p_dels": p_dels, "p_inss": p_inss,
         "p_ins_seq": letters,
         "applied": {"blocks": [(10 * (p + 1) + 5, 1000, 2 * A, 1) for p in range(P)] + [(10 * (2 * P + j + 1), 1000, A, 1) for j in range(V)], "nodes": nodes,
                     "new_blocks": [(p, 1, p, P + p, p * 2 * A) for p in range(P)], "member_src": member_src,
                     "block_map": np.concatenate([np.full(2 * P, asm.NONE, np.uint32), P + np.arange(V, dtype=np.uint32)])}}
    first = offsets(s_counts)                                                      # what merged_blocks takes: the anchor halves, the append halves
    take = lambda src, col: src[first[0, col]:first[P * A - 1, col] + s_counts[P * A - 1, col]]
    anchor = {"cons": [cons] * P, "n_members": [A] * P, "node_ids": nid[:P * A], "counts": s_counts[:P * A], "subs": take(s_subs, 0), "dels": take(s_dels, 1),
              "inss": take(s_inss, 2), "ins_seq": letters}
    append = {"n_members": [A] * P, "node_ids": nid[P * A:nk], "res": np.concatenate([r_counts.astype(np.int64), offsets(r_counts)], axis=1), "subs": p_subs, "dels": p_dels,
              "inss": p_inss, "ins_seq": letters}
    return t, anchor, append


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("promises", 2000), ("depth", 64), ("survivors", 4000), ("subs", 20), ("dels", 3), ("inss", 3), ("letters", 6)):
        ap.add_argument("--" + name, type=int, default=default)
    a = ap.parse_args()
    t, anchor, append = build(a)
    K = asm.Tables(t)
    res = {"promises": a.promises, "depth": a.depth, "survivors": a.survivors}
    for flags, name in ((asm.MERGED_ONLY, "merged_only_ms"), (0, "default_ms")):
        for timed in (False, True):                                             # a warm-up, then the call
            clock = time.perf_counter()
            out = asm.assemble_blocks_raw(*K.call_args(), flags=flags, keep=K, ins_seq_len=len(K.L))
            wall = time.perf_counter() - clock
            if timed:
                res[name] = round(wall * 1e3, 2)
                res["members" if flags else "members_all"], res["subs" if flags else "subs_all"] = out.out.n_members, out.out.n_subs
                if flags:
                    res["stream_ms"] = [round(x, 2) for x in asm.last_ms()]
                    got = out.to_arrays()
            out.free()
    dt.merged_blocks(anchor, append)
    clock = time.perf_counter()
    want = dt.merged_blocks(anchor, append)
    res["host_ms"] = round((time.perf_counter() - clock) * 1e3, 2)
    res["same"] = bool(got["counts"].tolist() == want["counts"].tolist() and got["subs"].tobytes() == want["subs"].tobytes() and got["dels"].tobytes() == want["dels"].tobytes()
                       and got["inss"]["len"].tolist() == want["inss"]["len"].tolist() and [w[0] for w in got["who"]] == want["node_ids"].tolist())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
