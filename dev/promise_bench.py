"""SURVEY 8(f)-1, the whole step at merge scale: pga_solve_promises (consensus + edits + CIGAR in, member sequences built on the device)
against pga_map_variations on the SAME members with sequences and bands built beforehand -- the parent route without the host's own build
time, i.e. its floor.  Wall time of the C calls alone (the ctypes packing of either binding is outside the window), the two alternating.
usage: dev/promise_bench.py [n_members] [block_len] [repeats]"""
import sys, os, time, json, ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import mapvarbind as mb
import promise_ref as pr
from pangraph_amd import mapvar, promise

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = bytes.maketrans(b"ACGTYRWSKMDVHBN-", b"TGCARYWSMKHBDVN-")


def member(rng, cons):
    """(edit, sequence): 1 % substitutions and a few short indels, the edit lists sorted by position and apart from each other"""
    L = len(cons)
    cuts = sorted(int(x) for x in rng.choice(np.arange(1, L // 40 - 1), int(rng.integers(0, 5)), replace=False) * 40)   # indel sites, 40 apart at least
    dels, inss = [], []
    for c in cuts:
        if rng.random() < 0.5:
            dels.append((c, int(rng.integers(1, 20))))
        else:
            inss.append((c, mb.random_seq(rng, int(rng.integers(1, 20)))))
    a = cons.copy()
    k = np.flatnonzero(rng.random(L) < 0.01)
    k = k[~np.isin(k // 40, [c // 40 for c in cuts])]                    # no substitution next to an indel
    alt = ACGT[rng.integers(0, 4, len(k))]
    keep = alt != a[k]
    k, alt = k[keep], alt[keep]
    a[k] = alt
    parts, at = [], 0
    for pos, what in sorted([(p, n) for p, n in dels] + [(p, s) for p, s in inss], key=lambda t: t[0]):
        parts.append(a[at:pos]); at = pos
        if isinstance(what, int):
            at = pos + what
        else:
            parts.append(np.frombuffer(what.encode(), dtype=np.uint8))
    parts.append(a[at:])
    e = {"subs": [(int(p), chr(c)) for p, c in zip(k, alt)], "dels": dels, "inss": inss}
    return e, np.concatenate(parts).tobytes().decode()


if __name__ == "__main__":
    n_members = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    L = int(sys.argv[2]) if len(sys.argv) > 2 else 10000
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    rng = np.random.default_rng(20261018)
    dll = C.CDLL(os.path.join(ROOT, "pangraph_amd", "libpgalign.so"))
    promises, jobs = [], []
    while sum(len(q[4]) for q in promises) < n_members:
        depth = min(int(rng.choice([50, 100, 200, 500, 1000])), n_members - sum(len(q[4]) for q in promises))
        reverse = len(promises) % 2 == 1
        cons = ACGT[rng.integers(0, 4, int(L * rng.uniform(0.8, 1.2)))]
        append = cons.tobytes().decode()
        oriented = append.encode().translate(COMP)[::-1].decode() if reverse else append
        cut, n = len(oriented) // 3, int(rng.integers(1, 30))                # the anchor: the oriented append consensus without n letters
        anchor = oriented[:cut] + oriented[cut + n:]
        cigar = [(cut, "M"), (n, "I"), (len(oriented) - cut - n, "M")]
        cband = mb.band_from_edits(pr.from_cigar(cigar), len(anchor))
        members = []
        for _ in range(depth):
            e, seq = member(rng, cons)
            members.append(e)
            if reverse:
                seq, eo = seq.encode().translate(COMP)[::-1].decode(), pr.edit_reverse_complement(e, len(append))
            else:
                eo = e
            band = mb.band_from_edits(eo, len(append))
            jobs.append((anchor, seq, band[0] + cband[0], band[1] + cband[1]))
        promises.append((anchor, append, reverse, cigar, members))
    p = mapvar.params()
    # ---- both calls packed once; the window holds the C call alone ----
    K = promise._Packed(promises)
    R1 = (mapvar.res_t * K.n_mem)()
    keep = {}
    J = (mapvar.job_t * len(jobs))()
    for i, j in enumerate(jobs):
        rb = keep.setdefault(j[0], j[0].encode()); qb = keep.setdefault((i, "q"), j[1].encode())
        J[i].ref = rb; J[i].qry = qb; J[i].ref_len = len(rb); J[i].qry_len = len(qb); J[i].mean_shift = j[2]; J[i].band_width = j[3]
    R2 = (mapvar.res_t * len(jobs))()
    outs = lambda: (C.POINTER(mapvar.sub_t)(), C.POINTER(mapvar.del_t)(), C.POINTER(mapvar.ins_t)(), C.POINTER(C.c_char)())
    dll.pga_solve_promises.restype = C.c_int; dll.pga_map_variations.restype = C.c_int
    dll.pga_solve_promises.argtypes = [C.c_int64] + [C.c_void_p] * 12
    dll.pga_map_variations.argtypes = [C.c_int64] + [C.c_void_p] * 7
    dll.pga_free.argtypes = [C.c_void_p]
    dll.pga_last_error.restype = C.c_char_p

    def run(which):
        o = outs()
        t0 = time.perf_counter()
        if which == 0:
            rc = dll.pga_solve_promises(*K.args(), C.byref(p), R1, *[C.byref(x) for x in o])
        else:
            rc = dll.pga_map_variations(len(jobs), J, C.byref(p), R2, *[C.byref(x) for x in o])
        dt = time.perf_counter() - t0                                        # both calls end in a device synchronise and a download
        assert rc == 0, dll.pga_last_error()
        return dt, o

    def unpack(R, o, m):
        r = R[m]
        base = C.addressof(o[3].contents)
        return (r.status, r.score, r.attempts, r.hit_boundary, [(o[0][r.sub_off + k].pos, o[0][r.sub_off + k].alt) for k in range(r.n_subs)],
                [(o[1][r.del_off + k].pos, o[1][r.del_off + k].len) for k in range(r.n_dels)],
                [(o[2][r.ins_off + k].pos, C.string_at(base + o[2][r.ins_off + k].seq_off, o[2][r.ins_off + k].len)) for k in range(r.n_inss)])

    times = [[], []]
    same = None
    for it in range(repeats + 1):                                            # the first round of both is the warm-up
        res = [run(0), run(1)] if it % 2 == 0 else [run(1), run(0)][::-1]
        if it == 0:
            idx = range(0, len(jobs), max(1, len(jobs) // 500))
            same = all(unpack(R1, res[0][1], m) == unpack(R2, res[1][1], m) for m in idx)
            statuses = sorted(set(R1[m].status for m in range(K.n_mem)))
        else:
            times[0].append(res[0][0]); times[1].append(res[1][0])
        for _, o in res:
            for x in o:
                dll.pga_free(C.cast(x, C.c_void_p))
    med = [float(np.median(t)) for t in times]
    print(json.dumps(dict(members=len(jobs), promises=len(promises), member_Mbp=round(sum(len(j[1]) for j in jobs) / 1e6, 1), repeats=repeats,
                          solve_promises_s=dict(median=round(med[0], 4), min=round(min(times[0]), 4), max=round(max(times[0]), 4)),
                          map_variations_on_built_sequences_s=dict(median=round(med[1], 4), min=round(min(times[1]), 4), max=round(max(times[1]), 4)),
                          bytes_handed_over=dict(solve_promises=K.handed_over + 4 * sum(len(q[3]) for q in promises),
                                                 map_variations=sum(len(v) for v in keep.values()) + 32 * len(jobs)),
                          identical_on_sample=same, statuses=statuses)))
