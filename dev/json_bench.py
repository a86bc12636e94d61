"""pga_export_json at pangenome-like sizes, once each after a warm-up:
  plasmids   tests/golden/plasmids.json.gz replicated to about --gb of text (ids shifted per replica, the insertion letters shared)
  blocks     a synthetic block-heavy graph: --blocks blocks of --depth members, every member with 5 subs, a del and an insertion of 8 letters
  long_ins   --long insertions of --letters letters each, with the insertion chunk of the library (64 letters per item) and with one item
             per insertion (PGA_JSON_INS_CHUNK): what splitting a long insertion over threads is worth
    python dev/json_bench.py [--gb 1.0] [--blocks 100000 --depth 10] [--long 2000 --letters 100000] [--only plasmids|blocks|long_ins]
Prints one JSON line per workload: sizes and n_bytes; for a sink that discards its input and one that writes to /dev/null: call_ms (the
whole call on the host's clock), mb_per_s = n_bytes / call_ms, and the pga_json_last_ms split: tables_ms (first upload to the layout),
tile_kernel_ms, host_copy_ms (consensus letters, names, descriptions into the pinned tiles), sink_ms; verdict_ms: the call without a sink.
Beside it, on the same machine: host_mb_per_s, json_write_str on the unreplicated plasmids (the restatement is linear in the graph), and
gfa_ms / gfa_mb_per_s, pga_export_gfa with sequences on the same graph arrays."""
import argparse
import ctypes as C
import gzip
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pangraph_amd import batch  # noqa: E402
from pangraph_amd import gfa, jsonout  # noqa: E402
from pangraph_amd.mapvar import del_t, ins_t, sub_t  # noqa: E402
from pangraph_amd.reconsensus import rc_member_t  # noqa: E402
from pangraph_amd.topology import topo_block_t, topo_node_t, topo_path_t  # noqa: E402

RC_BLOCK = np.dtype([("consensus", "<u8"), ("cons_len", "<u4"), ("n_members", "<u4")])          # pga_rc_block_t (numpy has no dtype for its pointer)
ptr = lambda x: C.c_void_p(x.ctypes.data) if len(x) else None


class Arrays:
    """the arrays of one call as numpy records; graph_args / block_args point into them"""

    def __init__(self, B, P, N, R, M, S, D, I, L, meta, keep=None):
        self.B, self.P, self.N, self.R, self.M, self.S, self.D, self.I, self.L, self.path_meta, self.keep = B, P, N, R, M, S, D, I, L, meta, keep
        self.graph_args = (len(B), ptr(B), len(P), ptr(P), len(N), ptr(N))
        self.block_args = (len(B), ptr(R), ptr(M), ptr(S), ptr(D), ptr(I), ptr(L))
        self.ins_seq_len = len(L)


def plasmids(gb):
    G = json.load(gzip.open(os.path.join(ROOT, "tests", "golden", "plasmids.json.gz")))
    F = jsonout.json_from_json(G)
    one = len(jsonout.json_write_str(G))
    reps = max(1, min(1023, round(gb * 1e9 / one)))
    view = lambda a, ct, n: np.frombuffer(a, np.dtype(ct), n).copy()
    nb, np_, nn = F.graph_args[0], F.graph_args[2], F.graph_args[4]
    B, P, N = view(F.graph_args[1], topo_block_t, nb), view(F.graph_args[3], topo_path_t, np_), view(F.graph_args[5], topo_node_t, nn)
    n_mem = sum(F.B[b].n_members for b in range(nb))
    R, M = np.frombuffer(F.B, RC_BLOCK, nb).copy(), view(F.M, rc_member_t, n_mem)
    S, D, I = (view(a, ct, int(M[f].sum())) for a, ct, f in ((F.S, sub_t, "n_subs"), (F.D, del_t, "n_dels"), (F.I, ins_t, "n_inss")))
    Bs, Ps, Ns = np.tile(B, reps), np.tile(P, reps), np.tile(N, reps)
    r_b, r_p, r_n = (np.repeat(np.arange(reps, dtype=np.uint64), n) for n in (nb, np_, nn))
    Bs["block_id"] = (Bs["block_id"] >> np.uint64(10)) + (r_b << np.uint64(54))              # ascending over the replicas, 17-20 digits as hashed ids are
    Ns["node_id"] = (Ns["node_id"] >> np.uint64(10)) + (r_n << np.uint64(54))
    Ns["block"] += (r_n * np.uint64(nb)).astype(np.uint32)
    Ps["path_id"] += r_p * np.uint64(np_)
    Ps["node_off"] += r_p * np.uint64(nn)
    meta = [(m[0], b"%s_%d" % (m[1], r), m[2]) for r in range(reps) for m in F.path_meta]
    L = np.frombuffer(F.L, np.uint8, F.ins_seq_len).copy()
    return Arrays(Bs, Ps, Ns, np.tile(R, reps), np.tile(M, reps), np.tile(S, reps), np.tile(D, reps), np.tile(I, reps), L, meta, keep=F), G


def synthetic(n_blocks, depth, n_subs=5, n_dels=1, n_inss=1, ins_len=8, cons_len=200):
    rng = np.random.default_rng(11)
    n = n_blocks * depth
    B = np.zeros(n_blocks, np.dtype(topo_block_t))
    B["block_id"] = np.unique(rng.integers(1, 1 << 63, 2 * n_blocks, dtype=np.uint64))[:n_blocks]
    B["cons_len"], B["depth"], B["alive"] = cons_len, depth, 1
    N = np.zeros(n, np.dtype(topo_node_t))
    N["node_id"] = rng.permutation(np.unique(rng.integers(1, 1 << 63, 2 * n, dtype=np.uint64))[:n])
    N["block"], N["member"] = np.arange(n) % n_blocks, np.arange(n) // n_blocks             # path p visits every block once: its member slot is p
    N["reverse"], N["pos0"], N["pos1"] = rng.integers(0, 2, n), np.arange(n) * cons_len, (np.arange(n) + 1) * cons_len
    P = np.zeros(depth, np.dtype(topo_path_t))
    P["path_id"], P["node_off"], P["n_nodes"], P["circular"] = np.arange(depth), np.arange(depth, dtype=np.uint64) * n_blocks, n_blocks, 1
    cons = C.create_string_buffer((b"ACGTTGCAAC" * (cons_len // 10 + 1))[:cons_len], cons_len)
    R = np.zeros(n_blocks, RC_BLOCK)
    R["consensus"], R["cons_len"], R["n_members"] = C.addressof(cons), cons_len, depth
    M = np.zeros(n, np.dtype(rc_member_t))
    M["n_subs"], M["n_dels"], M["n_inss"] = n_subs, n_dels, n_inss
    S = np.zeros(n * n_subs, np.dtype(sub_t)); D = np.zeros(n * n_dels, np.dtype(del_t)); I = np.zeros(n * n_inss, np.dtype(ins_t))
    S["pos"], S["alt"] = rng.integers(0, cons_len, len(S)), np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, len(S))]
    D["pos"], D["len"] = rng.integers(0, cons_len - 8, len(D)), rng.integers(1, 8, len(D))
    L = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, max(min(len(I) * ins_len, 1 << 26), ins_len, 1))].copy()      # (long insertions share letters)
    I["pos"], I["len"] = rng.integers(0, cons_len, len(I)), ins_len
    I["seq_off"] = (np.arange(len(I), dtype=np.uint64) * np.uint64(ins_len)) % np.uint64(len(L) - ins_len + 1)
    meta = [(n_blocks * cons_len, b"genome_%d" % p, None) for p in range(depth)]
    return Arrays(B, P, N, R, M, S, D, I, L, meta, keep=cons)


def run(A, dll, chunk=None):
    """-> {"n_bytes", "discard": {...}, "devnull": {...}, "verdict_ms"}"""
    args, keep = jsonout.marshal(A.graph_args, A.block_args, A.path_meta, A.ins_seq_len)
    null = os.open(os.devnull, os.O_WRONLY)
    sinks = {"discard": gfa.SINK(lambda ctx, at, n: 0), "devnull": gfa.SINK(lambda ctx, at, n: 0 if os.write(null, (C.c_char * n).from_address(at)) == n else 1), "verdict": None}
    if chunk is not None:
        os.environ["PGA_JSON_INS_CHUNK"] = str(chunk)

    def call(sink):
        out = jsonout.json_out_t()
        t = time.perf_counter()
        rc = dll.pga_export_json(*args, 0, C.byref(out), C.cast(sink, C.c_void_p) if sink is not None else None, None)
        dt = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError(dll.pga_last_error().decode())
        n_bytes = out.n_bytes
        dll.pga_json_free(C.byref(out))
        return dt, n_bytes, jsonout.last_ms(dll)
    res = {}
    try:
        for name, sink in sinks.items():
            call(sink)                                                          # a warm-up, then the call
            dt, n_bytes, ms = call(sink)
            if name == "verdict":
                res["verdict_ms"] = round(dt, 2)
                continue
            res[name] = {"call_ms": round(dt, 2), "mb_per_s": round(n_bytes / dt / 1e3, 1), "tables_ms": round(ms[0], 3), "tile_kernel_ms": round(ms[1], 3), "host_copy_ms": round(ms[2], 3),
                         "sink_ms": round(ms[3], 3)}
        res["n_bytes"] = n_bytes
    finally:
        os.environ.pop("PGA_JSON_INS_CHUNK", None)
        os.close(null)
    return res


def gfa_on(A, dll):
    """pga_export_gfa with sequences on the same graph arrays, a discarding sink -> (ms, n_bytes)"""
    gfa._bind(dll)
    nb = len(A.B)
    cons = (C.c_void_p * nb)(*[int(x) for x in A.R["consensus"]])
    names_p, names_l, keep = gfa._bytes_array([m[1] for m in A.path_meta], len(A.P))
    prm = gfa.GfaParams(include_sequences=True).to_c()
    sink = gfa.SINK(lambda ctx, at, n: 0)
    for _ in range(2):
        out = gfa.gfa_out_t()
        t = time.perf_counter()
        rc = dll.pga_export_gfa(*A.graph_args, C.cast(cons, C.c_void_p), gfa._ptr(names_p), gfa._ptr(names_l), C.cast(C.byref(prm), C.c_void_p), 0, C.byref(out), C.cast(sink, C.c_void_p), None)
        dt = (time.perf_counter() - t) * 1e3
        if rc != 0:
            raise RuntimeError(dll.pga_last_error().decode())
        n_bytes = out.n_bytes
        dll.pga_gfa_free(C.byref(out))
    return dt, n_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=1.0)
    for name, default in (("blocks", 100000), ("depth", 10), ("long", 2000), ("letters", 100000)):
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--only", choices=("plasmids", "blocks", "long_ins"))
    a = ap.parse_args()
    dll = batch.lib()
    jsonout._bind(dll)
    if a.only in (None, "plasmids"):
        A, G = plasmids(a.gb)
        res = {"workload": "plasmids", "replicas": len(A.P) // len(G["paths"]), "paths": len(A.P), "blocks": len(A.B), "nodes": len(A.N), "subs": len(A.S), "dels": len(A.D), "inss": len(A.I)}
        res.update(run(A, dll))
        t = time.perf_counter()
        text = jsonout.json_write_str(G)
        res["host_mb_per_s"] = round(len(text) / (time.perf_counter() - t) / 1e6, 2)
        ms, n = gfa_on(A, dll)
        res.update(gfa_ms=round(ms, 2), gfa_n_bytes=n, gfa_mb_per_s=round(n / ms / 1e3, 1), same_bytes_unreplicated=jsonout.export_json(G, dll=dll) == text)
        print(json.dumps(res), flush=True)
    if a.only in (None, "blocks"):
        A = synthetic(a.blocks, a.depth)
        res = {"workload": "blocks", "paths": len(A.P), "blocks": len(A.B), "nodes": len(A.N), "subs": len(A.S), "dels": len(A.D), "inss": len(A.I)}
        res.update(run(A, dll))
        ms, n = gfa_on(A, dll)
        res.update(gfa_ms=round(ms, 2), gfa_n_bytes=n, gfa_mb_per_s=round(n / ms / 1e3, 1))
        print(json.dumps(res), flush=True)
    if a.only in (None, "long_ins"):
        A = synthetic(a.long, 1, n_subs=0, n_dels=0, n_inss=1, ins_len=a.letters, cons_len=10)
        res = {"workload": "long_ins", "insertions": len(A.I), "letters_each": a.letters}
        for label, chunk in (("chunk_64", None), ("one_item_per_insertion", 1 << 30)):
            r = run(A, dll, chunk)
            res[label] = {"call_ms": r["discard"]["call_ms"], "tile_kernel_ms": r["discard"]["tile_kernel_ms"], "tables_ms": r["discard"]["tables_ms"]}
            res["n_bytes"] = r["n_bytes"]
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
