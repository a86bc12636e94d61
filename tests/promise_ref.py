"""MergePromise::solve_promise (packages/pangraph/src/pangraph/reweave.rs:40-94) restated for the tests, composed from the helpers of
mapvarbind.py (apply_edit, band_from_edits): what the reference has worked out for every member when it calls map_variations.  New
pieces: the complement table (io/seq.rs:9-33), Edit::reverse_complement (edits.rs:257-276), Edit::from_cigar (edits.rs:538-566), the band
sum (map_variations.rs:23-26) and the order of the statuses (include/pga_align.h, pga_solve_promises)."""
import mapvarbind as mb

COMPLEMENT = dict(zip("ACGTYRWSKMDVHBN-", "TGCARYWSMKHBDVN-"))          # io/seq.rs:9-29; anything else is an error


class Rejected(Exception):
    pass


def complement(c):
    if c not in COMPLEMENT:
        raise Rejected(f"Unknown nucleotide character: '{c}'")
    return COMPLEMENT[c]


def reverse_complement(seq):
    return "".join(complement(c) for c in reversed(seq))


def edit_reverse_complement(e, ln):
    """Edit::reverse_complement: every list mapped, then sort_by_key(pos) -- a stable sort"""
    subs = sorted([(ln - pos - 1, complement(a)) for pos, a in e["subs"]], key=lambda t: t[0])
    dels = sorted([(ln - pos - n, n) for pos, n in e["dels"]], key=lambda t: t[0])
    inss = sorted([(ln - pos, reverse_complement(s)) for pos, s in e["inss"]], key=lambda t: t[0])
    return {"subs": subs, "dels": dels, "inss": inss}


def parse_cigar(text):
    """'10M2D5M' -> [(10, 'M'), (2, 'D'), (5, 'M')]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append((int(n), ch)); n = ""
    return out


def from_cigar(ops):
    """Edit::from_cigar: M = X advance, I an insertion of N's at the current position, D a deletion that advances"""
    rpos, inss, dels = 0, [], []
    for ln, op in ops:
        if op in "M=X":
            rpos += ln
        elif op == "I":
            inss.append((rpos, "N" * ln))
        elif op == "D":
            dels.append((rpos, ln)); rpos += ln
        else:
            raise NotImplementedError(f"Unsupported CIGAR operation: {op}")
    return {"subs": [], "dels": dels, "inss": inss}


def cigar_from_alignment(ref_aln, qry_aln):
    """the CIGAR ([(len, op)], M I D) of a gapped pair of rows"""
    ops = []
    for r, q in zip(ref_aln, qry_aln):
        op = "I" if r == "-" else "D" if q == "-" else "M"
        if ops and ops[-1][1] == op:
            ops[-1] = (ops[-1][0] + 1, op)
        else:
            ops.append((1, op))
    return ops


def stage_promise(promise):
    """-> [(status, mean_shift, band_width, oriented seq)] per member: 0 / 7 / 8 / 9 as pga_stage_promise_jobs reports them
    (band 0, 0 and seq "" where the status is not 0; the empty member: 0, 0, 0, "")"""
    anchor, append, reverse, cigar_ops, members = promise
    cband = mb.band_from_edits(from_cigar(cigar_ops), len(anchor))
    out = []
    for e in members:
        if cband is None:                                               # reweave.rs:47: fails before the loop
            out.append((8, 0, 0, "")); continue
        seq = mb.apply_edit(append, e)
        if seq == "":
            out.append((0, 0, 0, "")); continue
        try:
            if reverse:
                seq, e = reverse_complement(seq), edit_reverse_complement(e, len(append))
        except Rejected:
            out.append((9, 0, 0, "")); continue
        band = mb.band_from_edits(e, len(append))
        if band is None:
            out.append((7, 0, 0, "")); continue
        out.append((0, band[0] + cband[0], band[1] + cband[1], seq))
    return out


def solve_promise(oracle_dll, promise, p=None):
    """-> one dict per member as oracle_map_variations returns them; status 7 / 8 / 9 and the empty member carry no alignment fields"""
    anchor = promise[0]
    out = []
    for st, ms, bw, seq in stage_promise(promise):
        if st != 0:
            out.append(dict(status=st, score=0, attempts=0, hit_boundary=0, subs=[], dels=[], inss=[]))
        elif seq == "":
            out.append(dict(status=0, score=0, attempts=0, hit_boundary=0, subs=[], dels=[(0, len(anchor))], inss=[]))
        else:
            out.append(mb.oracle_map_variations(oracle_dll, anchor, seq, ms, bw, p))
    return out
