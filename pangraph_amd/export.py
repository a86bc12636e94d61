"""The host side of the two exports of a finished graph, export block-sequences (PangraphBlock::sequences,
packages/pangraph/src/pangraph/pangraph_block.rs:135-189) and export core-genome (core_block_aln with concatenate_records,
commands/export/export_core_genome.rs:53-141): the loader that turns a pangraph JSON and a guide strain into the arrays a core alignment is
built from, in the layout of pangraph_amd.reconstruct.  The device entries are not built yet (DESIGN.md section 0, row ex)."""
from .reconstruct import graph_from_json


def core_from_json(g, guide_name):
    """a pangraph JSON (as reconstruct.graph_from_json takes it) and the guide strain's name -> (args, keys, in_record_order): args, a
    dict: blocks as reconstruct takes them, member_path[m] = the path index of global member m, n_paths, guide_path = the guide's path
    index, guide_nodes = its nodes in path.nodes order as (block index, member index inside the block, reverse); keys[p], the record key of path p (its
    name, or its id as a string: pangraph_block.rs:170); in_record_order(rows), the rows as the reference emits its records: sorted by key
    (concatenate_records collects them in a BTreeMap<String, _>; equal keys stay in path order here, merging them is the caller's)."""
    if isinstance(g, str):
        import gzip
        import json
        with (gzip.open(g, "rt") if g.endswith(".gz") else open(g)) as f:
            g = json.load(f)
    blocks, paths, names = graph_from_json(g)
    path_ids = sorted(g["paths"], key=int)
    keys = [n if n is not None else str(int(pid)) for n, pid in zip(names, path_ids)]
    member_path = [None] * sum(len(b["members"]) for b in blocks)
    first = [0]
    for b in blocks:
        first.append(first[-1] + len(b["members"]))
    for p, path in enumerate(paths):
        for blk, mem, _ in path["nodes"]:
            member_path[first[blk] + mem] = p
    if None in member_path:
        raise ValueError("a block member that no path visits")
    if guide_name not in names:
        raise KeyError(f"path {guide_name!r} not found in graph")       # (path_id_by_name, pangraph.rs:258-268)
    guide = names.index(guide_name)
    args = dict(blocks=blocks, member_path=member_path, n_paths=len(paths), guide_path=guide, guide_nodes=list(paths[guide]["nodes"]))

    def in_record_order(rows):
        return [rows[p] for p in sorted(range(len(keys)), key=lambda p: keys[p].encode())]
    return args, keys, in_record_order
