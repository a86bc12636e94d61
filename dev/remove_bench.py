"""One pga_remove_paths call at a simplify-like size -- many genomes, a handful of focal ones -- against the remove_path loop of
simplify() on the same graph, once each after a warm-up, and against a device-to-device copy of the bytes the kernels have to move.
Default: 1000 paths of 2000 nodes over 20000 blocks, 1 % of the paths kept; every member has 3 substitutions, every second a deletion,
every third an insertion of 8 letters.
    python dev/remove_bench.py [--paths 1000 --nodes 2000 --blocks 20000 --keep 0.01] [--letters] [--no-host]
Prints one JSON line: sizes; call_ms (the whole call on the host's clock); upload_ms, kernels_ms (with the waits between them), download_ms
(the stream's clock, pga_remove_last_ms); kernel_bytes = the graph arrays, the member counts and the kept list entries read once plus every output array written once,
and kernel_gbps = kernel_bytes / kernels_ms; memcpy_gbps: one hipMemcpy device to device of kernel_bytes / 2 bytes (it reads and writes as
many) in the same run; host_ms: the remove_path loop on the dict graph."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import remove as rm  # noqa: E402
from pangraph_amd import simplify as sp  # noqa: E402
from pangraph_amd.mapvar import del_t, ins_t, sub_t  # noqa: E402
from pangraph_amd.reconsensus import rc_member_t  # noqa: E402
from pangraph_amd.topology import topo_block_t, topo_node_t, topo_path_t  # noqa: E402

RC_BLOCK = np.dtype([("consensus", "<u8"), ("cons_len", "<u4"), ("n_members", "<u4")])


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
    cons = np.frombuffer(b"ACGTTGCAAC" * 9, np.uint8).copy()
    R = np.zeros(a.blocks, RC_BLOCK)
    R["consensus"], R["cons_len"], R["n_members"] = cons.ctypes.data, 90, depth
    m = np.arange(n)
    M = np.zeros(n, np.dtype(rc_member_t))
    M["n_subs"], M["n_dels"], M["n_inss"] = 3, m % 2 == 0, m % 3 == 0
    so, do, io = np.repeat(m, M["n_subs"]), np.repeat(m, M["n_dels"]), np.repeat(m, M["n_inss"])
    S = np.zeros(len(so), np.dtype(sub_t)); S["pos"], S["alt"] = (so * 7 + np.arange(len(so))) % 90, 65
    D = np.zeros(len(do), np.dtype(del_t)); D["pos"], D["len"] = do % 80, 2
    I = np.zeros(len(io), np.dtype(ins_t)); I["pos"], I["len"], I["seq_off"] = io % 91, 8, np.arange(len(io), dtype=np.uint64) * 8
    seq = np.tile(np.frombuffer(b"ACGTACGT", np.uint8), len(io))
    keep = np.zeros(a.paths, np.uint8)
    keep[rng.choice(a.paths, max(1, int(round(a.paths * a.keep))), replace=False)] = 1
    return {"B": B, "P": P, "N": N, "R": R, "M": M, "S": S, "D": D, "I": I, "seq": seq, "keep": keep, "cons": cons, "order": order, "first": first}


def host_graph(a, G):
    """the same graph as simplify.normalize leaves it (an edit is one shared object: remove_path does not look inside)"""
    bid = G["B"]["block_id"].tolist()
    g = {"paths": {}, "nodes": {}, "blocks": {b: {"consensus": "A" * 90, "alignments": {}} for b in bid}}
    ids, blk = G["N"]["node_id"].tolist(), G["N"]["block"].tolist()
    for k in range(a.paths):
        pid = k + 1
        g["paths"][pid] = {"nodes": ids[k * a.nodes:(k + 1) * a.nodes], "tot_len": 0, "circular": bool(G["P"]["circular"][k]), "name": str(pid)}
        for i in range(k * a.nodes, (k + 1) * a.nodes):
            g["nodes"][ids[i]] = {"block_id": bid[blk[i]], "path_id": pid, "strand": "+", "position": (0, 0)}
            g["blocks"][bid[blk[i]]]["alignments"][ids[i]] = None
    return g


def memcpy_gbps(n_bytes):
    """one device-to-device copy of n_bytes through the HIP runtime the library is linked against, timed by events after a warm-up copy"""
    hip = C.CDLL("libamdhip64.so")
    check = lambda rc: rc == 0 or (_ for _ in ()).throw(RuntimeError(f"HIP error {rc}"))
    src, dst, e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()
    check(hip.hipMalloc(C.byref(src), C.c_size_t(n_bytes))); check(hip.hipMalloc(C.byref(dst), C.c_size_t(n_bytes)))
    check(hip.hipEventCreate(C.byref(e0))); check(hip.hipEventCreate(C.byref(e1)))
    try:
        check(hip.hipMemset(src, 0, C.c_size_t(n_bytes)))
        check(hip.hipMemcpy(dst, src, C.c_size_t(n_bytes), 3))                 # hipMemcpyDeviceToDevice; the warm-up
        check(hip.hipDeviceSynchronize())
        check(hip.hipEventRecord(e0, None))
        check(hip.hipMemcpyAsync(dst, src, C.c_size_t(n_bytes), 3, None))
        check(hip.hipEventRecord(e1, None))
        check(hip.hipEventSynchronize(e1))
        check(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    finally:
        hip.hipEventDestroy(e0); hip.hipEventDestroy(e1); hip.hipFree(src); hip.hipFree(dst)
    return 2 * n_bytes / (ms.value * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    for name, default in (("paths", 1000), ("nodes", 2000), ("blocks", 20000)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--keep", type=float, default=0.01)
    ap.add_argument("--letters", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    G = build(a)
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    args = (len(G["B"]), ptr(G["B"]), len(G["P"]), ptr(G["P"]), len(G["N"]), ptr(G["N"]))
    block_args = (len(G["B"]), ptr(G["R"]), ptr(G["M"]), ptr(G["S"]), ptr(G["D"]), ptr(G["I"]), ptr(G["seq"]))
    keep = (C.c_uint8 * a.paths).from_buffer(G["keep"])
    flags = rm.COMPACT_LETTERS if a.letters else 0
    res = {"paths": a.paths, "nodes_per_path": a.nodes, "blocks": a.blocks, "kept_paths": int(G["keep"].sum()), "members": len(G["M"]),
           "subs": len(G["S"]), "dels": len(G["D"]), "inss": len(G["I"]), "letters": bool(a.letters)}
    dll = batch.lib()
    for timed in (False, True):                                                 # a warm-up, then the call
        t = time.perf_counter()
        out = rm.remove_paths_raw(args, block_args, keep, flags, len(G["seq"]), dll)
        dt = time.perf_counter() - t
        o = out.out
        after = (o.n_nodes, o.n_members, o.n_dead_blocks, o.n_subs, o.n_dels, o.n_inss, o.n_ins_letters)
        first_path = [o.nodes[i].node_id for i in range(o.paths[0].n_nodes)]
        out.free()
        if timed:
            up, kern, down = rm.last_ms(dll)
            res.update(call_ms=round(dt * 1e3, 2), upload_ms=round(up, 3), kernels_ms=round(kern, 3), download_ms=round(down, 3))
    res.update(nodes_after=after[0], members_after=after[1], dead_blocks_after=after[2])
    n_in = sum(G[k].nbytes for k in ("B", "P", "N", "M", "keep")) + (after[3] + after[4]) * 8 + after[5] * 16 + after[6]      # (of the lists only what is kept is read)
    n_out = G["B"].nbytes + after[0] * 40 + after[1] * 12 + len(G["M"]) * 8 + (after[3] + after[4]) * 8 + after[5] * 16 + after[6]
    res["kernel_bytes"] = int(n_in + n_out)
    res["kernel_gbps"] = round(res["kernel_bytes"] / (res["kernels_ms"] * 1e-3) / 1e9, 2)
    res["memcpy_gbps"] = round(memcpy_gbps(res["kernel_bytes"] // 2), 2)
    if not a.no_host:
        g = host_graph(a, G)
        kept = {str(k + 1) for k in np.flatnonzero(G["keep"]).tolist()}
        t = time.perf_counter()
        for pid in [pid for pid in sorted(g["paths"]) if g["paths"][pid]["name"] not in kept]:
            sp.remove_path(g, pid)
        res["host_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        res["same_first_path"] = g["paths"][min(g["paths"])]["nodes"] == first_path and len(g["nodes"]) == after[0] and len(g["blocks"]) == a.blocks - after[2]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
