"""export block-sequences and export core-genome restated for the tests, line by line, in the graph shape of pangraph_amd.export.core_from_json
(blocks = [{"consensus", "members": [edit]}], member_path[m] = the path index of global member m, guide_nodes = [(block, member, reverse)]):
  apply_aligned        Edit::apply_aligned        packages/pangraph/src/pangraph/edits.rs:331-347
  sequences            PangraphBlock::sequences   pangraph_block.rs:135-189
  core_block_ids       Pangraph::core_block_ids   pangraph.rs:235-255
  core_block_aln       core_block_aln             commands/export/export_core_genome.rs:53-107
  concatenate_records  concatenate_records        export_core_genome.rs:109-141
Edit::apply is mapvarbind.apply_edit and the complement promise_ref.reverse_complement, as in reconstruct_ref.  New pieces: in expected_results the statuses
and call failures a device entry for the two exports is to report (0 built; 2 a letter the complement rejects; 3 a literal '-' in
unaligned mode, which Edit::apply would strip; inconsistent input fails the call)."""
import mapvarbind as mb
import promise_ref as pr
import reconstruct_ref as rr


class ExportError(Exception):
    """the reference returns Err"""


class CallFailure(Exception):
    """the entry fails the call (the reference panics, or the input contradicts itself)"""


def apply_aligned(ref, e):
    """edits.rs:331-347: substitutions in list order, then every deleted position becomes '-'; insertions are missing"""
    q = list(ref)
    for pos, alt in e["subs"]:
        q[pos] = alt
    for pos, ln in e["dels"]:
        for k in range(pos, pos + ln):
            q[k] = "-"
    return "".join(q)


def sequences(block, names, aligned):
    """pangraph_block.rs:135-189 with RecordNaming::Path: one (name, seq) per member in alignments() order; names[j] is the record name
    of member j's path"""
    out = []
    for j, edits in enumerate(block["members"]):
        seq = apply_aligned(block["consensus"], edits) if aligned else mb.apply_edit(block["consensus"], edits)
        out.append((names[j], seq))
    return out


def member_first(blocks):
    first = [0]
    for b in blocks:
        first.append(first[-1] + len(b["members"]))
    return first


def core_block_ids(blocks, member_path, n_paths):
    """pangraph.rs:235-255: the blocks present exactly once in each path"""
    first = member_first(blocks)
    path_ids = set(range(n_paths))
    core = []
    for b, block in enumerate(blocks):
        block_path_ids = set(member_path[first[b]:first[b + 1]])
        n_nodes = len(block["members"])
        is_in_all_paths = block_path_ids == path_ids
        is_not_duplicated = n_nodes == len(block_path_ids)
        if is_in_all_paths and is_not_duplicated:
            core.append(b)
    return core


def concatenate_records(records_list):
    """export_core_genome.rs:109-141: records of one name are joined in the order they come; the output is sorted by name (a BTreeMap
    keyed by the name as a String: byte order)"""
    if not records_list:
        return []
    records = {name: "" for name, _ in records_list[0]}
    for entries in records_list:
        for name, seq in entries:
            if name not in records:
                raise ExportError(f"Sequence name '{name}' not found in the initial set. This is an internal error. Please report it to developers.")
            records[name] += seq
    return [(name, records[name]) for name in sorted(records, key=lambda s: s.encode())]


def core_block_aln(blocks, member_path, keys, guide_path, guide_nodes, aligned):
    """export_core_genome.rs:53-107; keys[p]: the record name of path p (its name, or its id as a string) -> [(name, seq)] sorted by name"""
    first = member_first(blocks)
    core = core_block_ids(blocks, member_path, len(keys))
    records = []
    for bid, _, reverse in guide_nodes:
        if bid not in core:
            continue
        block_records = sequences(blocks[bid], [keys[member_path[first[bid] + j]] for j in range(len(blocks[bid]["members"]))], aligned)
        if reverse:
            try:
                block_records = [(name, pr.reverse_complement(seq)) for name, seq in block_records]
            except pr.Rejected as e:
                raise ExportError(str(e))
        records.append(block_records)
    if not records:
        return [(k, "") for k in keys]
    return concatenate_records(records)


# ---------------------------------------------------------------- what the entries report
def _check_edits(blocks):
    for b in blocks:
        L = len(b["consensus"])
        for e in b["members"]:
            for pos, alt in e["subs"]:
                if pos >= L:
                    raise CallFailure("substitution beyond the consensus")
                if ord(alt) > 255:
                    raise CallFailure("substitution letter outside one byte")
            for pos, ln in e["dels"]:
                if pos + ln > L:
                    raise CallFailure("deletion beyond the consensus")
            for pos, _ in e["inss"]:
                if pos > L:
                    raise CallFailure("insertion beyond the consensus")


def _piece(block, e, reverse, aligned):
    """one (member, reverse) piece -> (letters as the entry would emit them or None, flags): the letters before Edit::apply strips a '-'"""
    s = apply_aligned(block["consensus"], e) if aligned else rr._apply_keeping_gaps(block["consensus"], e)
    bad = reverse and any(c not in pr.COMPLEMENT for c in s)
    gap = (not aligned) and "-" in s
    if not bad and reverse:
        s = pr.reverse_complement(s)
    return s, bad, gap


def _row(pieces, aligned):
    parts = [_piece(blk, e, rev, aligned) for blk, e, rev in pieces]
    out = dict(status=0, len=sum(len(s) for s, _, _ in parts), seq=None)
    if any(bad for _, bad, _ in parts):
        out["status"] = 2
    elif any(gap for _, _, gap in parts):
        out["status"] = 3
    else:
        out["seq"] = "".join(s for s, _, _ in parts)
        if out["len"] > (1 << 31):
            raise CallFailure("row over 2^31 letters")
    return out


def expected_block_sequences(blocks, aligned=True):
    """one row per member in global member order: status, len, seq; a status 0 row is checked against `sequences` above"""
    _check_edits(blocks)
    rows = []
    for block in blocks:
        ref = sequences(block, [None] * len(block["members"]), aligned)
        for j, e in enumerate(block["members"]):
            r = _row([(block, e, False)], aligned)
            assert r["status"] in (0, 3)
            if r["status"] == 0:
                assert r["seq"] == ref[j][1]
            rows.append(r)
    return rows


def expected_results(blocks, member_path, n_paths, guide_path, guide_nodes, aligned=True):
    """the core alignment as (rows in path-index order, core = the core blocks in guide order with the guide's strand and first column); the call failures are CallFailure.  Where every
    row has status 0 the rows are checked against core_block_aln above (with the path index as the record name)."""
    _check_edits(blocks)
    first = member_first(blocks)
    if n_paths == 0:
        return [], []
    if any(p >= n_paths for p in member_path):
        raise CallFailure("member_path names a path that does not exist")
    if not 0 <= guide_path < n_paths:
        raise CallFailure("guide_path names a path that does not exist")
    core_ids = core_block_ids(blocks, member_path, n_paths)
    core, col, named = [], 0, set()
    for bid, mem, reverse in guide_nodes:
        if not (0 <= bid < len(blocks) and 0 <= mem < len(blocks[bid]["members"])):
            raise CallFailure("guide node names a member that does not exist")
        if member_path[first[bid] + mem] != guide_path:
            raise CallFailure("guide node whose member is not on guide_path")
        if bid not in core_ids:
            continue
        if bid in named:
            raise CallFailure("core block named twice by the guide nodes")
        named.add(bid)
        core.append(dict(block=bid, reverse=bool(reverse), col=col, cons_len=len(blocks[bid]["consensus"])))
        col += len(blocks[bid]["consensus"])
    if named != set(core_ids):
        raise CallFailure("core block not named by the guide nodes")
    rows = []
    for p in range(n_paths):
        pieces = []
        for c in core:
            blk = blocks[c["block"]]
            j = member_path[first[c["block"]]:first[c["block"] + 1]].index(p)
            pieces.append((blk, blk["members"][j], c["reverse"], ))
        rows.append(_row(pieces, aligned))
    keys = ["%09d" % p for p in range(n_paths)]                           # (names whose byte order is the path order)
    if all(r["status"] == 0 for r in rows):
        assert [(k, r["seq"]) for k, r in zip(keys, rows)] == core_block_aln(blocks, member_path, keys, guide_path, guide_nodes, aligned)
    elif any(r["status"] == 2 for r in rows):
        try:
            core_block_aln(blocks, member_path, keys, guide_path, guide_nodes, aligned)
            raise AssertionError("the restatement does not fail where a status says the reference does")
        except ExportError:
            pass
    return rows, core
