"""One pga_apply_merge call at a build-like size against the dict loop at the end of reweave(update=None) on the same input, once each after a
warm-up.  Default: 1000 paths of 5000 nodes over 20000 blocks, 3000 of them cut into 3 unaligned intervals, every member kept.
    python dev/apply_bench.py [--paths 1000 --nodes 5000 --blocks 20000 --cut 3000 --intervals 3] [--no-host]
Prints one JSON line: sizes, device_ms (the call: uploads, kernels, downloads), host_ms (reweave() with its plan and slices handed in)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pangraph_amd import apply as ap  # noqa: E402
from pangraph_amd import reweave as rw  # noqa: E402
from pangraph_amd.reweave import plan_interval_t  # noqa: E402
from pangraph_amd.slice import slice_member_t, slice_res_t  # noqa: E402
from pangraph_amd.topology import topo_block_t, topo_node_t, topo_path_t  # noqa: E402


def build(a):
    rng = np.random.default_rng(7)
    n = a.paths * a.nodes
    block = rng.integers(0, a.blocks, n, dtype=np.uint32)
    block[:a.blocks] = np.arange(a.blocks, dtype=np.uint32)                     # every block has a node
    rng.shuffle(block)
    nid = (np.arange(1, n + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(1)      # distinct, 63 bits
    order = np.lexsort((nid, block))                                            # the members of a block by node id
    depth = np.bincount(block, minlength=a.blocks).astype(np.uint32)
    first = np.concatenate(([0], np.cumsum(depth)[:-1])).astype(np.int64)
    member = np.empty(n, np.uint32)
    member[order] = (np.arange(n) - first[block[order]]).astype(np.uint32)
    N = np.zeros(n, np.dtype(topo_node_t))
    N["node_id"], N["block"], N["member"], N["reverse"] = nid, block, member, rng.integers(0, 2, n)
    N["pos0"] = np.tile(np.arange(a.nodes, dtype=np.uint64) * 100, a.paths)
    N["pos1"] = N["pos0"] + 90
    B = np.zeros(a.blocks, np.dtype(topo_block_t))
    B["block_id"], B["cons_len"], B["depth"], B["alive"] = np.arange(1, a.blocks + 1, dtype=np.uint64) * 1000, 90, depth, 1
    P = np.zeros(a.paths, np.dtype(topo_path_t))
    P["path_id"], P["node_off"], P["n_nodes"], P["circular"] = np.arange(1, a.paths + 1), np.arange(a.paths, dtype=np.uint64) * a.nodes, a.nodes, rng.integers(0, 2, a.paths)
    cut_blocks = np.sort(rng.choice(a.blocks, a.cut, replace=False)).astype(np.uint32)
    K = np.zeros(a.cut, np.dtype(ap.apply_cut_t))
    K["block"], K["n_intervals"], K["first_interval"] = cut_blocks, a.intervals, np.arange(a.cut, dtype=np.uint64) * a.intervals
    ni = a.cut * a.intervals
    ln = 90 // a.intervals
    I = np.zeros(ni, np.dtype(plan_interval_t))
    I["new_block_id"] = np.arange(ni, dtype=np.uint64) * 1000 + 7               # (no multiple of 1000: none equals a surviving id)
    I["start"] = np.tile(np.arange(a.intervals, dtype=np.uint32) * ln, a.cut)
    I["end"], I["match"] = I["start"] + ln, -1
    kept = np.repeat(depth[cut_blocks], a.intervals)
    S = np.zeros(ni, np.dtype(slice_res_t))
    moff = np.concatenate(([0], np.cumsum(kept)[:-1])).astype(np.int64)
    S["n_kept"], S["member_off"] = kept, moff
    nm = int(kept.sum())
    M = np.zeros(nm, np.dtype(slice_member_t))
    s_of = np.repeat(np.arange(ni), kept)
    M["member"] = np.arange(nm) - moff[s_of]
    old = order[first[np.repeat(cut_blocks, a.intervals)][s_of] + M["member"].astype(np.int64)]      # the position of the old node of every kept member
    M["reverse"] = N["reverse"][old]
    M["pos_start"] = N["pos0"][old] + I["start"][s_of]
    M["pos_end"] = N["pos0"][old] + I["end"][s_of]
    return B, P, N, K, I, S, M, old


def host_side(a, B, P, N, K, I, S, M):
    """the same input as reweave() takes it: the dict graph, and the plan and slices as its two stand-ins return them"""
    bid = B["block_id"].tolist()
    g = {"paths": {}, "nodes": {}, "blocks": {b: {"consensus": "A" * 90, "alignments": {}} for b in bid}}
    ids, blk, p0, p1, rev = N["node_id"].tolist(), N["block"].tolist(), N["pos0"].tolist(), N["pos1"].tolist(), N["reverse"].tolist()
    for k in range(a.paths):
        pid = k + 1
        g["paths"][pid] = {"nodes": ids[k * a.nodes:(k + 1) * a.nodes], "tot_len": 0, "circular": bool(P["circular"][k]), "name": None}
        for i in range(k * a.nodes, (k + 1) * a.nodes):
            g["nodes"][ids[i]] = {"block_id": bid[blk[i]], "path_id": pid, "strand": "-" if rev[i] else "+", "position": (p0[i], p1[i])}
            g["blocks"][bid[blk[i]]]["alignments"][ids[i]] = None
    cut_ids = [bid[b] for b in K["block"].tolist()]
    ivs = [{"start": s, "end": e, "aligned": 0, "new_block_id": n, "is_anchor": 0} for s, e, n in zip(I["start"].tolist(), I["end"].tolist(), I["new_block_id"].tolist())]
    p = {"n_failed": 0, "blocks": [{"block": k, "n_intervals": a.intervals, "first_interval": k * a.intervals, "status": 0} for k in range(a.cut)], "intervals": ivs,
         "slice_intervals": [(v["start"], v["end"], 0) for v in ivs], "promises": []}
    mm, mr, ma, mb = M["member"].tolist(), M["reverse"].tolist(), M["pos_start"].tolist(), M["pos_end"].tolist()
    rows, s = [], 0
    for k in range(a.cut):
        per = []
        for _ in range(a.intervals):
            off, n = int(S["member_off"][s]), int(S["n_kept"][s])
            per.append({"kept": [dict(member=mm[x], reverse=bool(mr[x]), pos=(ma[x], mb[x]), subs=(), dels=(), inss=()) for x in range(off, off + n)], "dropped": []})
            s += 1
        rows.append(per)
    return g, [{"qry": b, "ref": b} for b in cut_ids], p, rows


def main():
    ap_ = argparse.ArgumentParser()
    for name, default in (("paths", 1000), ("nodes", 5000), ("blocks", 20000), ("cut", 3000), ("intervals", 3)):
        ap_.add_argument("--" + name, type=int, default=default)
    ap_.add_argument("--no-host", action="store_true")
    a = ap_.parse_args()
    B, P, N, K, I, S, M, _ = build(a)
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    args = (len(B), ptr(B), len(P), ptr(P), len(N), ptr(N))
    res = {"paths": a.paths, "nodes_per_path": a.nodes, "blocks": a.blocks, "cut": a.cut, "intervals": a.intervals, "members": len(M)}
    for timed in (False, True):                                                 # a warm-up, then the call
        t = time.perf_counter()
        out = ap.apply_merge_raw(args, len(K), ptr(K), ptr(I), ptr(S), ptr(M))
        dt = time.perf_counter() - t
        res["nodes_after"] = out.out.n_nodes
        first = [out.out.nodes[i].node_id for i in range(out.out.paths[0].n_nodes)]
        out.free()
        if timed:
            res["device_ms"] = round(dt * 1e3, 2)
    if not a.no_host:
        g, matches, p, rows = host_side(a, B, P, N, K, I, S, M)
        t = time.perf_counter()
        g, _ = rw.reweave(g, matches, 0, plan=lambda *x: p, slicer=lambda bl: rows)
        res["host_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        res["same_first_path"] = g["paths"][1]["nodes"] == first
    print(json.dumps(res))


if __name__ == "__main__":
    main()
