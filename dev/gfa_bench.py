"""One pga_export_gfa call at a pangenome-like size against the host restatement gfa.gfa_tables on the same graph, once each after a
warm-up, and against a device-to-device copy of the file's bytes.  Default: 1000 paths of 5000 nodes over 20000 blocks of 90 letters.
    python dev/gfa_bench.py [--paths 1000 --nodes 5000 --blocks 20000] [--sequences] [--no-host]
Prints one JSON line: sizes and n_bytes; for a sink that discards its input and one that writes to /dev/null: call_ms (the whole call on
the host's clock), tables_ms (the stream's clock from the first upload to the tables: verdict mode's share), tile_kernel_ms (the tile
kernels on the stream's clock), host_copy_ms (consensus letters and names into the pinned tiles) and sink_ms (pga_gfa_last_ms);
tile_gbps = n_bytes / tile_kernel_ms and memcpy_gbps: one hipMemcpy device to device of n_bytes in the same run (it reads and writes as
many), kernel_share = the tile kernel's rate as a share of it; verdict_ms: the call without a sink; host_ms: gfa_tables on the lists."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import gfa  # noqa: E402
from pangraph_amd.topology import topo_block_t, topo_node_t, topo_path_t  # noqa: E402


def build(a):
    rng = np.random.default_rng(7)
    n = a.paths * a.nodes
    block = rng.integers(0, a.blocks, n, dtype=np.uint32)
    block[:a.blocks] = np.arange(a.blocks, dtype=np.uint32)                     # every block has a node
    rng.shuffle(block)
    order = np.argsort(block, kind="stable")                                    # the members of a block in node order
    depth = np.bincount(block, minlength=a.blocks).astype(np.uint32)
    first = np.concatenate(([0], np.cumsum(depth)[:-1])).astype(np.int64)
    member = np.empty(n, np.uint32)
    member[order] = (np.arange(n) - first[block[order]]).astype(np.uint32)
    N = np.zeros(n, np.dtype(topo_node_t))
    N["node_id"], N["block"], N["member"], N["reverse"] = np.arange(1, n + 1), block, member, rng.integers(0, 2, n)
    B = np.zeros(a.blocks, np.dtype(topo_block_t))
    B["block_id"] = np.unique(rng.integers(1, 1 << 63, 2 * a.blocks, dtype=np.uint64))[:a.blocks]      # ascending, 17-19 digits as hashed BlockIds are
    B["cons_len"], B["depth"], B["alive"] = 90, depth, 1
    P = np.zeros(a.paths, np.dtype(topo_path_t))
    P["path_id"], P["node_off"], P["n_nodes"], P["circular"] = np.arange(1, a.paths + 1), np.arange(a.paths, dtype=np.uint64) * a.nodes, a.nodes, rng.integers(0, 2, a.paths)
    return B, P, N


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
    for name, default in (("paths", 1000), ("nodes", 5000), ("blocks", 20000)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--sequences", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    B, P, N = build(a)
    ptr = lambda x: C.c_void_p(x.ctypes.data)
    args = (len(B), ptr(B), len(P), ptr(P), len(N), ptr(N))
    cons = [b"ACGTTGCAAC" * 9] * a.blocks if a.sequences else None
    names = [b"genome_%d" % k for k in range(a.paths)]
    params = gfa.GfaParams(include_sequences=a.sequences)
    dll = batch.lib()
    gfa._bind(dll)
    dll.pga_gfa_last_ms.restype, dll.pga_gfa_last_ms.argtypes = None, [C.POINTER(C.c_double)]
    cons_p, _, keep_c = gfa._bytes_array(cons, a.blocks)
    names_p, names_l, keep_n = gfa._bytes_array(names, a.paths)
    prm = params.to_c()
    null = os.open(os.devnull, os.O_WRONLY)
    sinks = {"discard": gfa.SINK(lambda ctx, at, n: 0), "devnull": gfa.SINK(lambda ctx, at, n: 0 if os.write(null, (C.c_char * n).from_address(at)) == n else 1), "verdict": None}

    def call(sink):
        out = gfa.gfa_out_t()
        t = time.perf_counter()
        rc = dll.pga_export_gfa(*args, gfa._ptr(cons_p), gfa._ptr(names_p), gfa._ptr(names_l), C.cast(C.byref(prm), C.c_void_p), 0, C.byref(out),
                                C.cast(sink, C.c_void_p) if sink is not None else None, None)
        dt = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError(dll.pga_last_error().decode())
        sizes = (out.n_segments, out.n_links, out.n_paths, out.n_steps, out.n_bytes)
        dll.pga_gfa_free(C.byref(out))
        ms = (C.c_double * 4)()
        dll.pga_gfa_last_ms(ms)
        return dt, sizes, tuple(ms)

    res = {"paths": a.paths, "nodes_per_path": a.nodes, "blocks": a.blocks, "include_sequences": bool(a.sequences), "tile_kb": int(os.environ.get("PGA_EXPORT_TILE_KB", 16384))}
    for name, sink in sinks.items():
        call(sink)                                                              # a warm-up, then the call
        dt, sizes, ms = call(sink)
        if name == "verdict":
            res["verdict_ms"] = round(dt, 2)
            continue
        res[name] = {"call_ms": round(dt, 2), "tables_ms": round(ms[0], 3), "tile_kernel_ms": round(ms[1], 3), "host_copy_ms": round(ms[2], 3), "sink_ms": round(ms[3], 3)}
    res.update(segments=sizes[0], links=sizes[1], steps=sizes[3], n_bytes=sizes[4])
    res["tile_gbps"] = round(sizes[4] / (res["discard"]["tile_kernel_ms"] * 1e-3) / 1e9, 2)
    res["memcpy_gbps"] = round(memcpy_gbps(sizes[4]) / 2, 2)                     # (bytes written per second: the copy writes n_bytes and reads as many)
    res["kernel_share"] = round(res["tile_gbps"] / res["memcpy_gbps"], 4)
    if not a.no_host:
        lists = ([tuple(r)[:4] for r in B.tolist()], [tuple(r) for r in P.tolist()], [tuple(r)[:6] for r in N.tolist()])
        t = time.perf_counter()
        exp = gfa.gfa_tables(*lists, params, cons, names)
        res["host_ms"] = round((time.perf_counter() - t) * 1e3, 1)
        pieces = []
        gfa.export_gfa_raw(args, cons, names, params, pieces.append, dll=dll).free()
        res["same_bytes"] = b"".join(pieces) == exp["text"]
    os.close(null)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
