"""One round of the path side of `pangraph simplify`, both ways, on one generated graph:
  host    the host functions of pangraph_amd/simplify.py as simplify() drives them: find_transitive_edges + choose_round + per chosen edge
          orient_merging_edge and find_node_pairings + per chosen edge graph_merging_update (Python dicts; every path is walked once per edge)
  device  one pga_plan_simplify call (validation, host-to-device, kernels, sort, the host's choice of the round, device-to-host: wall time
          of the C call alone, which ends behind its last synchronisation)
Shape: n_paths circular genomes over the same n_core core blocks in the same order (a genome is laid reversed with probability 0.3); between
two core blocks an accessory block that a random half of the genomes carry, so that no edge between whole blocks is transitive; a fraction
`cut` of the core blocks is cut into two pieces on every genome: those are the transitive edges, all of depth n_paths.
The first repetitions of both are the warm-up; the result line carries the graph's size, the medians and the spread.
usage: dev/topo_bench.py [n_paths=200] [n_core=250] [cut=0.25] [host_repeats=3] [device_repeats=20]"""
import sys, os, time, json, copy, random, statistics, ctypes as C
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pangraph_amd import batch, simplify as sp, topology as tp


def build(n_paths, n_core, cut, seed=20261019):
    rng = random.Random(seed)
    blocks, units = {}, []                                   # a unit: the blocks a genome lays for one core position, forward
    bid = 0
    for k in range(n_core):
        pieces = 2 if rng.random() < cut else 1
        unit = []
        for _ in range(pieces):
            bid += 1
            blocks[bid] = {"consensus": "A" * rng.randint(200, 2000), "alignments": {}}
            unit.append((bid, rng.choice("+-")))
        bid += 1
        blocks[bid] = {"consensus": "A" * rng.randint(50, 500), "alignments": {}}
        units.append((unit, bid))
    g = {"paths": {}, "nodes": {}, "blocks": blocks}
    nid = 0
    flip = {"+": "-", "-": "+"}
    for p in range(n_paths):
        laid = []
        for k, (unit, acc) in enumerate(units):
            laid += unit
            if (p + k) % 2 == 0 if k % 7 == 0 else rng.random() < 0.5:       # (every seventh junction: exactly the genomes of one parity)
                laid.append((acc, "+"))
        if rng.random() < 0.3:
            laid = [(b, flip[s]) for b, s in reversed(laid)]
        path = g["paths"][p + 1] = {"nodes": [], "tot_len": 0, "circular": True, "name": f"g{p}"}
        at = 0
        for b, s in laid:
            nid += 1
            n = len(blocks[b]["consensus"])
            g["nodes"][nid] = {"block_id": b, "path_id": p + 1, "strand": s, "position": (at, at + n)}
            at += n
            blocks[b]["alignments"][nid] = None
            path["nodes"].append(nid)
    for b in [b for b, blk in blocks.items() if not blk["alignments"]]:
        del blocks[b]
    return g


def host_round(g):
    transitive = sp.find_transitive_edges(g)
    rnd = sp.choose_round(transitive)
    plans = []
    for e in rnd:
        e = sp.orient_merging_edge(g, e)
        pair, new = sp.find_node_pairings(g, e)
        plans.append((e, new))
    for e, new in plans:
        sp.graph_merging_update(g, e, {"consensus": "", "alignments": {}}, new)
    return len(transitive), len(rnd)


if __name__ == "__main__":
    arg = lambda i, d, t: t(sys.argv[i]) if len(sys.argv) > i else d
    n_paths, n_core, cut, host_repeats, device_repeats = arg(1, 200, int), arg(2, 250, int), arg(3, 0.25, float), arg(4, 3, int), arg(5, 20, int)
    dll = batch.lib()
    dll.pga_device_count.restype = C.c_int
    assert dll.pga_device_count() > 0, "no HIP device: nothing is measured"
    g = build(n_paths, n_core, cut)
    order = {b: sorted(blk["alignments"]) for b, blk in g["blocks"].items()}
    args = tp.pack_graph(g, order)
    t_host, t_dev, sizes = [], [], None
    for it in range(host_repeats + 1):
        h = copy.deepcopy(g)
        t0 = time.perf_counter()
        sizes = host_round(h)
        t1 = time.perf_counter()
        if it:
            t_host.append(t1 - t0)
    same = None
    for it in range(device_repeats + 3):
        t0 = time.perf_counter()
        out = tp.plan_round_raw(args, dll=dll)
        t1 = time.perf_counter()
        if it == 0:                                            # the two routes agree: the lists' sizes and every path's node ids
            o = out.out
            same = (o.n_transitive, o.n_round) == sizes and o.n_nodes == len(h["nodes"]) and all(
                [o.nodes[k].node_id for k in range(o.paths[i].node_off, o.paths[i].node_off + o.paths[i].n_nodes)] == h["paths"][o.paths[i].path_id]["nodes"] for i in range(o.n_paths))
        elif it >= 3:
            t_dev.append(t1 - t0)
        out.free()
    stat = lambda t: dict(median=round(statistics.median(t), 5), min=round(min(t), 5), max=round(max(t), 5))
    print(json.dumps(dict(paths=n_paths, nodes=len(g["nodes"]), blocks=len(g["blocks"]), transitive_edges=sizes[0], round_edges=sizes[1], host_repeats=host_repeats,
                          device_repeats=device_repeats, host_functions_s=stat(t_host), plan_simplify_s=stat(t_dev),
                          ratio=round(statistics.median(t_host) / statistics.median(t_dev), 1), identical=bool(same))))
