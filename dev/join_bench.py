"""Measurement only (not a test): pga_join_graphs on two children of the list_lengths, high_index and second_level sizes of tests/join_gen.py,
each call timed once after one warm-up call with the split of pga_join_last_ms, beside the dict route a host without the entry takes at a
guide-tree node for the same input: join.graph_join on the dicts, then close.graph_tables and the two flat layouts packed again.
Run on an MI355X:  python dev/join_bench.py"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import join_gen as jg  # noqa: E402
from pangraph_amd import batch, close as cl, join as jn  # noqa: E402


def device(k, label):
    dll = batch.lib()
    K = [jn.Tables(p["t"]) for p in k["parts"]]
    jn.join_graphs_raw(K, dll=dll).free()                                        # warm-up
    for flags in (0, jn.COPY_CONSENSUS):
        t0 = time.perf_counter()
        out = jn.join_graphs_raw(K, flags=flags, dll=dll)
        wall = (time.perf_counter() - t0) * 1e3
        ms = jn.last_ms(dll)
        o = out.out
        print(f"{label} flags={flags}: call {wall:.2f} ms (uploads {ms[0]:.2f}, kernels {ms[1]:.2f}, downloads {ms[2]:.2f}); after: {o.n_blocks} blocks, {o.n_paths} paths, "
              f"{o.n_nodes} nodes, {o.n_members} members, {o.n_subs} subs, {o.n_inss} inss, {o.n_ins_letters} letters, {o.n_cons_letters} consensus bytes owned")
        if flags == 0:
            print(f"{label}: against host_join: {jg.same(out.to_lists(), k['exp']) or 'same'}")
        out.free()


def dict_route(k, label):
    """graph_join on the dicts, then the two flat layouts packed again from the dicts (close.graph_tables, close.Tables)"""
    t0 = time.perf_counter()
    g = jn.graph_join(k["parts"][0]["g"], k["parts"][1]["g"])
    t1 = time.perf_counter()
    t, _ = cl.graph_tables(g)
    cl.Tables(t)
    t2 = time.perf_counter()
    print(f"{label}: dict route {1e3 * (t2 - t0):.1f} ms (graph_join {1e3 * (t1 - t0):.2f}, the flat arrays again {1e3 * (t2 - t1):.1f})")


if __name__ == "__main__":
    for name in ("list_lengths", "high_index", "second_level"):
        k = jg.case(name)
        device(k, name)
        dict_route(k, name)
