"""detach_unaligned_nodes (packages/pangraph/src/pangraph/detach_unaligned.rs:24-114) restated line by line for the tests, over
mapvarbind.apply_edit (Edit::apply, edits.rs:307-329) and promise_ref.reverse_complement (io/seq.rs:9-33), with a plain XXH64 for
utils/id.rs.  Graph shape as tests/simplify_ref.py: blocks {bid: {"consensus", "alignments": {nid: edit}}}, nodes {nid: {"block_id",
"path_id", "strand", "position"}}.  New pieces: the statuses of pga_detach_unaligned (include/pga_align.h), the array shape of its result,
and the tail of solve_promise (reweave.rs:88-93)."""
import struct

import mapvarbind as mb
import promise_ref as pr
import reconstruct_ref as rr

M64 = (1 << 64) - 1
P1, P2, P3, P4, P5 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _round(acc, lane):
    return (_rotl((acc + lane * P2) & M64, 31) * P1) & M64


def _merge(h, v):
    return ((h ^ _round(0, v)) * P1 + P4) & M64


def xxh64(data, seed=0):
    """XXH64 as its specification words it: stripes of 32 bytes into four accumulators, then 8, 4 and 1 byte steps, then the avalanche"""
    n, i = len(data), 0
    if n >= 32:
        acc = [(seed + P1 + P2) & M64, (seed + P2) & M64, seed, (seed - P1) & M64]
        while i + 32 <= n:
            lanes = struct.unpack_from("<4Q", data, i)
            acc = [_round(a, w) for a, w in zip(acc, lanes)]
            i += 32
        h = (_rotl(acc[0], 1) + _rotl(acc[1], 7) + _rotl(acc[2], 12) + _rotl(acc[3], 18)) & M64
        for a in acc:
            h = _merge(h, a)
    else:
        h = (seed + P5) & M64
    h = (h + n) & M64
    while i + 8 <= n:
        h = (_rotl(h ^ _round(0, struct.unpack_from("<Q", data, i)[0]), 27) * P1 + P4) & M64
        i += 8
    if i + 4 <= n:
        h = (_rotl(h ^ (struct.unpack_from("<I", data, i)[0] * P1 & M64), 23) * P2 + P3) & M64
        i += 4
    while i < n:
        h = (_rotl(h ^ (data[i] * P5 & M64), 11) * P1) & M64
        i += 1
    h ^= h >> 33
    h = h * P2 & M64
    h ^= h >> 29
    h = h * P3 & M64
    return h ^ (h >> 32)


def id_stream(node_id, seq):
    """(NodeId(usize), &Seq).hash(): usize::hash writes 8 little-endian bytes; Vec<AsciiChar>::hash writes the length as usize, then
    every AsciiChar(u8) as one byte"""
    return struct.pack("<Q", node_id) + struct.pack("<Q", len(seq)) + seq.encode("latin-1")


def block_id(node_id, seq):
    """utils/id.rs: XxHash64::with_seed(0)"""
    return xxh64(id_stream(node_id, seq), 0)


# ---------------------------------------------------------------- detach_unaligned.rs
def aligned_count(edit, cons_len):
    """edits.rs:439-442"""
    return max(cons_len - sum(ln for _, ln in edit["dels"]), 0)


def extract_unaligned_nodes(block):
    """detach_unaligned.rs:62-81; block is changed in place"""
    cons_len = len(block["consensus"])
    removed = [nid for nid in sorted(block["alignments"]) if aligned_count(block["alignments"][nid], cons_len) == 0]
    unaligned = []
    for nid in removed:
        edit = block["alignments"].pop(nid)
        unaligned.append((nid, mb.apply_edit(block["consensus"], edit)))
    return unaligned


def create_new_node_and_block(node_id, seq, old_node):
    """detach_unaligned.rs:86-114 -> (new node, new block id, new block); raises promise_ref.Rejected where the reference returns Err"""
    seq = seq if old_node["strand"] == "+" else pr.reverse_complement(seq)
    new_block_id = block_id(node_id, seq)
    new_block = {"consensus": seq, "alignments": {node_id: {"subs": [], "dels": [], "inss": []}}}      # PangraphBlock::from_consensus
    new_node = {"block_id": new_block_id, "path_id": old_node["path_id"], "strand": "+", "position": old_node["position"]}
    return new_node, new_block_id, new_block


def detach_unaligned_nodes(blocks, nodes):
    """detach_unaligned.rs:24-57; blocks: a list of (block id, block), extended in place; nodes: the nodes dictionary, changed in place"""
    unaligned = []
    for _, block in blocks:
        unaligned += extract_unaligned_nodes(block)
    for node_id, seq in unaligned:
        old = nodes.pop(node_id)
        new_node, bid, new_block = create_new_node_and_block(node_id, seq, old)
        blocks.append((bid, new_block))
        nodes[node_id] = new_node


# ---------------------------------------------------------------- what pga_detach_unaligned returns, in pangraph_amd.detach.detach_unaligned's shape
def expected_call(blocks, who):
    """blocks: [{"consensus", "members"}]; who: per block [(node_id, reverse)].  The restatement above does the work wherever the reference
    succeeds; an orphan it fails on (status 2) or strips a '-' from (status 3) keeps its slot, and its letters are not to be compared."""
    out_blocks, orphans, member_map = [], [], []
    flat, kept_total = 0, sum(1 for b in blocks for e in b["members"] if aligned_count(e, len(b["consensus"])) != 0)
    kept_at = 0
    for b, w in zip(blocks, who):
        blk = {"consensus": b["consensus"], "alignments": {k: e for k, e in enumerate(b["members"])}}          # (member order stands in for NodeId order)
        gone = dict(extract_unaligned_nodes(blk))
        out_blocks.append({"consensus": b["consensus"], "members": [blk["alignments"][k] for k in sorted(blk["alignments"])]})
        for k, e in enumerate(b["members"]):
            if k not in gone:
                member_map.append(kept_at); kept_at += 1
            else:
                node_id, reverse = w[k]
                raw = rr._apply_keeping_gaps(b["consensus"], e)
                status = 2 if reverse and any(c not in pr.COMPLEMENT for c in raw) else 3 if "-" in raw else 0
                o = {"member": flat + k, "node_id": node_id, "block": len(blocks) + len(orphans), "len": len(raw), "status": status, "block_id": 0, "seq": None}
                if status == 0:
                    node, bid, nb = create_new_node_and_block(node_id, gone[k], {"strand": "-" if reverse else "+", "path_id": 0, "position": (0, 0)})
                    assert len(nb["consensus"]) == len(raw) and node["strand"] == "+"
                    o["seq"], o["block_id"] = nb["consensus"], bid
                elif status == 2:
                    try:
                        create_new_node_and_block(node_id, gone[k], {"strand": "-", "path_id": 0, "position": (0, 0)})
                        raise AssertionError("the restatement does not fail where the status says the reference does")
                    except pr.Rejected:
                        pass
                member_map.append(kept_total + len(orphans))
                orphans.append(o)
        flat += len(b["members"])
    for o in orphans:
        out_blocks.append({"consensus": o["seq"], "members": [{"subs": [], "dels": [], "inss": []}]})
    return {"blocks": out_blocks, "orphans": orphans, "member_map": member_map}


# ---------------------------------------------------------------- solve_promise's tail
def merged_block(consensus, anchor_members, append_members):
    """reweave.rs:88-93: alignment_insert of every re-aligned member; both arguments {node id: edit} -> (node ids in BTreeMap order, edits)"""
    aln = dict(anchor_members)
    for nid, e in append_members.items():
        aln[nid] = e
    ids = sorted(aln)
    return ids, [aln[n] for n in ids]
