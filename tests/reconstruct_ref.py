"""reconstruct (packages/pangraph/src/commands/reconstruct/reconstruct_run.rs:78-127) restated for the tests over mapvarbind.apply_edit
(Edit::apply, edits.rs:307-329) and promise_ref.reverse_complement (io/seq.rs:9-33), in the graph shape pangraph_amd.reconstruct takes:
blocks = [{"consensus", "members": [edit]}], a path = {"nodes": [(block, member, reverse)], "tot_len", "first_pos"}.  New pieces: the order
of the statuses of pga_reconstruct (include/pga_align.h) and a plain letter-by-letter compare."""
import gzip

import mapvarbind as mb
import promise_ref as pr


def read_fasta(path):
    """a gzipped FASTA -> (names, sequences)"""
    names, seqs = [], []
    with gzip.open(path, "rt") as f:
        for line in f:
            if line.startswith(">"):
                names.append(line[1:].split()[0]); seqs.append([])
            else:
                seqs[-1].append(line.strip())
    return names, ["".join(s) for s in seqs]


class ReconError(Exception):
    """the reference returns Err"""


class Panic(Exception):
    """the reference panics"""


def rotate_right(seq, mid):
    """Vec::rotate_right (utils/string_rotate.rs): `assert!(k <= self.len())`, then the last k letters come first"""
    if mid > len(seq):
        raise Panic(f"rotate_right({mid}) of {len(seq)} letters")
    return seq[len(seq) - mid:] + seq[:len(seq) - mid]


def reconstruct_block_sequence(blocks, node):
    """reconstruct_run.rs:105-127"""
    blk, mem, reverse = node
    s = mb.apply_edit(blocks[blk]["consensus"], blocks[blk]["members"][mem])
    if reverse:
        try:
            s = pr.reverse_complement(s)
        except pr.Rejected as e:
            raise ReconError(str(e))
    return s


def reconstruct_path(blocks, path):
    """reconstruct_run.rs:78-103"""
    if path["nodes"]:
        first_node_pos = path["first_pos"]                                     # graph.nodes[first_node_id].position().0
        genome = "".join(reconstruct_block_sequence(blocks, n) for n in path["nodes"])
        if len(genome) != path["tot_len"]:
            raise ReconError(f"genome length mismatch: computed length {len(genome)} expected {path['tot_len']}")
        return rotate_right(genome, first_node_pos)
    return ""


def compare(a, b):
    """two sequences of one length -> (index of the first differing letter or -1, number of differing letters)"""
    assert len(a) == len(b)
    diff = [i for i, (x, y) in enumerate(zip(a, b)) if x != y]
    return (diff[0] if diff else -1, len(diff))


_GONE = None


def _apply_keeping_gaps(ref, e):
    """Edit::apply without its last step: deleted positions leave, a literal '-' stays (what pga_reconstruct would emit)"""
    q = list(ref)
    for pos, alt in e["subs"]:
        q[pos] = alt
    for pos, ln in e["dels"]:
        for k in range(pos, pos + ln):
            q[k] = _GONE
    for pos, seq in sorted(e["inss"], reverse=True):
        q[pos:pos] = list(seq)
    return "".join(c for c in q if c is not _GONE)


def expected_result(blocks, path, expected=None):
    """what pga_reconstruct reports for one path, as pangraph_amd.reconstruct.reconstruct returns it: the statuses in the order of
    include/pga_align.h (2 a rejected complement, 3 an emitted '-', 1 the length, 4 the rotation, 5 the expected length); status 0 is
    checked against reconstruct_path above"""
    out = dict(status=0, len=0, seq=None, first_mismatch=-1, n_mismatch=0)
    if not path["nodes"]:
        seq = ""
    else:
        parts = [(_apply_keeping_gaps(blocks[b]["consensus"], blocks[b]["members"][m]), rev) for b, m, rev in path["nodes"]]
        out["len"] = sum(len(s) for s, _ in parts)
        if any(rev and any(c not in pr.COMPLEMENT for c in s) for s, rev in parts):
            out["status"] = 2
        elif any("-" in s for s, _ in parts):
            out["status"] = 3
        elif out["len"] != path["tot_len"]:
            out["status"] = 1
        elif path["first_pos"] > out["len"]:
            out["status"] = 4
        if out["status"] in (1, 2):
            try:
                reconstruct_path(blocks, path)
                raise AssertionError("the restatement does not fail where the status says the reference does")
            except ReconError:
                pass
        if out["status"] == 4:
            try:
                reconstruct_path(blocks, path)
                raise AssertionError("the restatement does not panic where the status says the reference does")
            except Panic:
                pass
        if out["status"] != 0:
            return out
        seq = reconstruct_path(blocks, path)
        assert len(seq) == out["len"]
    if expected is not None and len(expected) != len(seq):
        out["status"] = 5
        return out
    out["seq"] = seq
    if expected is not None:
        out["first_mismatch"], out["n_mismatch"] = compare(seq, expected)
    return out


def expected_results(blocks, paths, expected=None, want_seqs=True):
    res = [expected_result(blocks, p, None if expected is None else expected[i]) for i, p in enumerate(paths)]
    if not want_seqs:
        for r in res:
            r["seq"] = None
    return res
