"""block_slice (packages/pangraph/src/pangraph/slice.rs:12-202) and Edit::is_empty_alignment (edits.rs:351-367) restated for the tests, line by
line: every interval filters every list, the coordinates are the reference's two loops, emptiness applies the edits and looks at what is left.
Deliberately without the closed forms of pga_slice.hip -- this is what the kernels are compared with.
An edit is {"subs": [(pos, letter)], "dels": [(pos, len)], "inss": [(pos, seq)]}; an interval is a dict with start, end, aligned, is_anchor,
reverse (the orientation; is_anchor and reverse are read only when aligned); a node is (pos_start, pos_end, path_len, reverse, circular)."""


class Panic(Exception):
    """where the reference panics (usize underflow, a failed sanity_check)"""


def interval(start, end, aligned=False, is_anchor=False, reverse=False):
    return dict(start=start, end=end, aligned=aligned, is_anchor=is_anchor, reverse=reverse)


def flip_of(i):
    """the `flip` of pga_slice_interval_t: whether new_strandedness reverses the strand"""
    return bool(i["aligned"] and not i["is_anchor"] and i["reverse"])


def contains(i, pos):                                      # utils/interval.rs:38-40
    return i["start"] <= pos and pos < i["end"]


def has_overlap_with(i, start, end):                       # utils/interval.rs:42-46
    return i["end"] > start and i["start"] < end


def insertion_overlap(i, pos, block_len):                  # pangraph_interval.rs:44-46
    return contains(i, pos) or (pos == block_len and i["end"] == block_len)


def slice_substitutions(i, S):
    return [(pos - i["start"], alt) for pos, alt in S if contains(i, pos)]


def slice_deletions(i, D):
    out = []
    for pos, ln in D:
        if has_overlap_with(i, pos, pos + ln):
            new_start = max(pos, i["start"]) - i["start"]
            new_end = min(pos + ln, i["end"]) - i["start"]
            out.append((new_start, new_end - new_start))
    return out


def slice_insertions(i, I, block_len):
    return [(pos - i["start"], seq) for pos, seq in I if insertion_overlap(i, pos, block_len)]


def slice_edits(i, ed, block_len):
    return {"inss": slice_insertions(i, ed["inss"], block_len), "dels": slice_deletions(i, ed["dels"]), "subs": slice_substitutions(i, ed["subs"])}


def new_strandedness(old_reverse, orientation_reverse, is_anchor):
    if is_anchor or not orientation_reverse:
        return old_reverse
    return not old_reverse


def _sub(a, b):
    if b > a:
        raise Panic("attempt to subtract with overflow")
    return a - b


def new_position_circular(old_position, node_coords, path_len, old_reverse):
    old_s, old_e = old_position
    s, e = node_coords
    if path_len == 0:
        raise Panic("remainder with a divisor of zero")
    if not old_reverse:
        return ((old_s + s) % path_len, (old_s + e) % path_len)
    return (_sub(old_e + path_len, e) % path_len, _sub(old_e + path_len, s) % path_len)


def new_position_non_circular(old_position, node_coords, old_reverse):
    old_s, old_e = old_position
    s, e = node_coords
    if not old_reverse:
        return (old_s + s, old_s + e)
    return (_sub(old_e, e), _sub(old_e, s))


def interval_node_coords(i, ed, block_len):
    s, e = i["start"], i["end"]
    for pos, ln in ed["dels"]:
        if pos <= i["start"]:
            s = _sub(s, min(ln + pos, i["start"]) - pos)
        if pos < i["end"]:
            e = _sub(e, min(ln + pos, i["end"]) - pos)
    for pos, seq in ed["inss"]:
        if pos < i["start"]:
            s += len(seq)
        if pos < i["end"]:
            e += len(seq)
        if pos == i["end"] and pos == block_len:
            e += len(seq)
    return (s, e)


def apply(ed, ref):
    """Edit::apply (edits.rs:307-329)"""
    q = list(ref)
    for pos, alt in ed["subs"]:
        q[pos] = alt
    for pos, ln in ed["dels"]:
        for k in range(pos, pos + ln):
            q[k] = "-"
    for pos, seq in sorted(ed["inss"], reverse=True):
        q[pos:pos] = list(seq)
    return "".join(c for c in q if c != "-")


def is_empty_alignment(ed, consensus):
    if sum(len(seq) for _, seq in ed["inss"]) > 0:
        return False
    if sum(ln for _, ln in ed["dels"]) < len(consensus):
        return False
    return len(apply(ed, consensus)) == 0


def sanity_check(ed, cons_len):
    if any(pos >= cons_len for pos, _ in ed["subs"]) or any(pos + ln > cons_len for pos, ln in ed["dels"]) or any(pos > cons_len for pos, _ in ed["inss"]):
        raise Panic("edit outside the consensus")


def block_slice(consensus, members, nodes, i):
    """-> (new consensus, kept, dropped): kept = one dict per member whose slice is not empty, in member order (member, reverse, node,
    pos, subs, dels, inss); dropped = the member indices with an empty slice (the None entries of node_updates)"""
    new_consensus = consensus[i["start"]:i["end"]]
    block_len = len(consensus)
    if block_len == 0:
        raise Panic("block of length 0")
    kept, dropped = [], []
    for m, (ed, node) in enumerate(zip(members, nodes)):
        sanity_check(ed, block_len)
        pos_start, pos_end, path_len, old_reverse, circular = node
        new_reverse = new_strandedness(old_reverse, i["reverse"], i["is_anchor"]) if i["aligned"] else old_reverse
        coords = interval_node_coords(i, ed, block_len)
        if circular:
            new_pos = new_position_circular((pos_start, pos_end), coords, path_len, old_reverse)
        else:
            new_pos = new_position_non_circular((pos_start, pos_end), coords, old_reverse)
        new_edits = slice_edits(i, ed, block_len)
        if is_empty_alignment(new_edits, new_consensus):
            dropped.append(m)
        else:
            kept.append(dict(member=m, reverse=bool(new_reverse), node=coords, pos=new_pos, **new_edits))
    return new_consensus, kept, dropped


def slice_blocks(blocks):
    """blocks as pangraph_amd.slice.slice_blocks takes them, but with this module's interval dicts -> the same nested lists: per block, per
    interval dict(kept=[...], dropped=[...])"""
    return [[dict(zip(("kept", "dropped"), block_slice(b["consensus"], b["members"], b["nodes"], i)[1:])) for i in b["intervals"]] for b in blocks]
