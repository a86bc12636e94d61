"""pga_merge_blocks at merge scale, end to end (validation, host-to-device, kernels, device-to-host: wall time of the C call alone), beside a
plain single-threaded host loop with the reference's structure (merge_blocks.rs:92-148 over pangraph_block.rs:63-75 and edits.rs:257-304: per
edge the two blocks are cloned, one of them complemented -- consensus, every edit mapped, every list sorted -- the right block's edits shifted
into a new Edit, and every member concatenated with a linear search per right insertion), compiled from the C below with gcc -O2.
Shape: n_edges edges over 2 * n_edges blocks of block_len letters (+-20 %), `depth` members each, ~0.1 % edits per member (a third each
substitutions, deletions of 1..20, insertions of 1..20, lists sorted by position); every second edge complements its right block; the
partner lists are random permutations.
usage: dev/simplify_bench.py [n_edges=1000] [depth=500] [block_len=10000] [repeats=5]"""
import sys, os, time, json, subprocess, tempfile, ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pangraph_amd import simplify as sp
from pangraph_amd.reconsensus import rc_block_t

HOST_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "pga_align.h"
typedef struct { uint32_t pos, len; char *seq; } hins_t;
typedef struct { pga_sub_t *subs; pga_del_t *dels; hins_t *inss; uint32_t ns, nd, ni; } hedit_t;
static char comp(char c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return c; } }
static void revcomp(char *s, uint32_t n) { for (uint32_t i = 0; i < n / 2; ++i) { char a = comp(s[i]); s[i] = comp(s[n - 1 - i]); s[n - 1 - i] = a; } if (n & 1) s[n / 2] = comp(s[n / 2]); }
/* a stable sort by position as a merge sort meets these lists: a strictly descending run is reversed, anything else is inserted entry by entry */
#define STABLE_SORT(T, a, n) do { int desc = 1; for (uint32_t i = 0; i + 1 < (n); ++i) if ((a)[i].pos <= (a)[i + 1].pos) { desc = 0; break; } \
	if (desc) { for (uint32_t i = 0; i < (n) / 2; ++i) { T t = (a)[i]; (a)[i] = (a)[(n) - 1 - i]; (a)[(n) - 1 - i] = t; } } \
	else for (uint32_t i = 1; i < (n); ++i) { T t = (a)[i]; uint32_t j = i; while (j && (a)[j - 1].pos > t.pos) { (a)[j] = (a)[j - 1]; --j; } (a)[j] = t; } } while (0)
static hedit_t clone_edit(const pga_rc_member_t c, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq)
{
	hedit_t e; e.ns = c.n_subs; e.nd = c.n_dels; e.ni = c.n_inss;
	e.subs = (pga_sub_t*)malloc((e.ns + 1) * sizeof(pga_sub_t)); memcpy(e.subs, subs, e.ns * sizeof(pga_sub_t));
	e.dels = (pga_del_t*)malloc((e.nd + 1) * sizeof(pga_del_t)); memcpy(e.dels, dels, e.nd * sizeof(pga_del_t));
	e.inss = (hins_t*)malloc((e.ni + 1) * sizeof(hins_t));
	for (uint32_t t = 0; t < e.ni; ++t) { e.inss[t].pos = inss[t].pos; e.inss[t].len = inss[t].len; e.inss[t].seq = (char*)malloc(inss[t].len + 1); memcpy(e.inss[t].seq, ins_seq + inss[t].seq_off, inss[t].len); }
	return e;
}
static void free_edit(hedit_t *e) { for (uint32_t t = 0; t < e->ni; ++t) free(e->inss[t].seq); free(e->subs); free(e->dels); free(e->inss); }
static void edit_revcomp(hedit_t *e, uint32_t len)
{
	for (uint32_t t = 0; t < e->ns; ++t) { e->subs[t].pos = len - e->subs[t].pos - 1; e->subs[t].alt = (uint32_t)comp((char)e->subs[t].alt); }
	for (uint32_t t = 0; t < e->nd; ++t) e->dels[t].pos = len - e->dels[t].pos - e->dels[t].len;
	for (uint32_t t = 0; t < e->ni; ++t) { e->inss[t].pos = len - e->inss[t].pos; revcomp(e->inss[t].seq, e->inss[t].len); }
	STABLE_SORT(pga_sub_t, e->subs, e->ns); STABLE_SORT(pga_del_t, e->dels, e->nd); STABLE_SORT(hins_t, e->inss, e->ni);
}
/* tot[4]: subs, dels, inss, inserted letters written */
void host_merge(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *mem, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq,
                int64_t n_edges, const pga_merge_edge_t *edges, const uint32_t *partner, char *o_cons, pga_rc_member_t *om, pga_sub_t *os, pga_del_t *od, pga_ins_t *oi, char *ol, uint64_t *tot)
{
	uint64_t *m0 = (uint64_t*)malloc((n_blocks + 1) * sizeof(uint64_t)), n_mem = 0;
	for (int64_t b = 0; b < n_blocks; ++b) { m0[b] = n_mem; n_mem += blocks[b].n_members; }
	uint64_t *s0 = (uint64_t*)malloc((n_mem + 1) * 3 * sizeof(uint64_t)), *d0 = s0 + n_mem + 1, *i0 = d0 + n_mem + 1;
	s0[0] = d0[0] = i0[0] = 0;
	for (uint64_t m = 0; m < n_mem; ++m) { s0[m + 1] = s0[m] + mem[m].n_subs; d0[m + 1] = d0[m] + mem[m].n_dels; i0[m + 1] = i0[m] + mem[m].n_inss; }
	uint64_t k = 0, ns = 0, nd = 0, ni = 0, nl = 0, nc = 0, p0 = 0;
	for (int64_t e = 0; e < n_edges; ++e) {
		const uint32_t bid[2] = {edges[e].left, edges[e].right};
		const int rc[2] = {edges[e].left_rc, edges[e].right_rc};
		const uint32_t depth = blocks[bid[0]].n_members;
		char *cons[2]; hedit_t *aln[2];
		for (int s = 0; s < 2; ++s) {                                       /* the block, cloned; reverse_complement() where asked for */
			const pga_rc_block_t B = blocks[bid[s]];
			cons[s] = (char*)malloc(B.cons_len + 1); memcpy(cons[s], B.consensus, B.cons_len);
			aln[s] = (hedit_t*)malloc((depth + 1) * sizeof(hedit_t));
			for (uint32_t m = 0; m < depth; ++m) { const uint64_t g = m0[bid[s]] + m; aln[s][m] = clone_edit(mem[g], subs + s0[g], dels + d0[g], inss + i0[g], ins_seq); }
			if (rc[s]) { revcomp(cons[s], B.cons_len); for (uint32_t m = 0; m < depth; ++m) edit_revcomp(&aln[s][m], B.cons_len); }
		}
		const uint32_t Ll = blocks[bid[0]].cons_len, Lr = blocks[bid[1]].cons_len;
		memcpy(o_cons + nc, cons[0], Ll); memcpy(o_cons + nc + Ll, cons[1], Lr); nc += Ll + Lr;
		for (uint32_t m = 0; m < depth; ++m) {
			hedit_t *a = &aln[0][m], *b = &aln[1][partner[p0 + m]];
			/* e2.shift(Ll): a new Edit */
			hedit_t sh; sh.ns = b->ns; sh.nd = b->nd; sh.ni = b->ni;
			sh.subs = (pga_sub_t*)malloc((sh.ns + 1) * sizeof(pga_sub_t)); sh.dels = (pga_del_t*)malloc((sh.nd + 1) * sizeof(pga_del_t)); sh.inss = (hins_t*)malloc((sh.ni + 1) * sizeof(hins_t));
			for (uint32_t t = 0; t < sh.ns; ++t) { sh.subs[t] = b->subs[t]; sh.subs[t].pos += Ll; }
			for (uint32_t t = 0; t < sh.nd; ++t) { sh.dels[t] = b->dels[t]; sh.dels[t].pos += Ll; }
			for (uint32_t t = 0; t < sh.ni; ++t) { sh.inss[t] = b->inss[t]; sh.inss[t].pos += Ll; sh.inss[t].seq = (char*)malloc(sh.inss[t].len + 1); memcpy(sh.inss[t].seq, b->inss[t].seq, sh.inss[t].len); }
			/* e1.concat(shifted) */
			hins_t *ci = (hins_t*)malloc((a->ni + sh.ni + 1) * sizeof(hins_t)); uint32_t cn = a->ni;
			for (uint32_t t = 0; t < a->ni; ++t) { ci[t] = a->inss[t]; ci[t].seq = (char*)malloc(ci[t].len + 1); memcpy(ci[t].seq, a->inss[t].seq, ci[t].len); }
			for (uint32_t t = 0; t < sh.ni; ++t) {
				uint32_t f = 0;
				while (f < cn && ci[f].pos != sh.inss[t].pos) ++f;
				if (f < cn) { ci[f].seq = (char*)realloc(ci[f].seq, ci[f].len + sh.inss[t].len + 1); memcpy(ci[f].seq + ci[f].len, sh.inss[t].seq, sh.inss[t].len); ci[f].len += sh.inss[t].len; }
				else { ci[cn] = sh.inss[t]; ci[cn].seq = (char*)malloc(sh.inss[t].len + 1); memcpy(ci[cn].seq, sh.inss[t].seq, sh.inss[t].len); ++cn; }
			}
			memcpy(os + ns, a->subs, a->ns * sizeof(pga_sub_t)); memcpy(os + ns + a->ns, sh.subs, sh.ns * sizeof(pga_sub_t));
			memcpy(od + nd, a->dels, a->nd * sizeof(pga_del_t)); memcpy(od + nd + a->nd, sh.dels, sh.nd * sizeof(pga_del_t));
			for (uint32_t t = 0; t < cn; ++t) { oi[ni + t].pos = ci[t].pos; oi[ni + t].len = ci[t].len; oi[ni + t].seq_off = nl; memcpy(ol + nl, ci[t].seq, ci[t].len); nl += ci[t].len; free(ci[t].seq); }
			om[k].n_subs = a->ns + sh.ns; om[k].n_dels = a->nd + sh.nd; om[k].n_inss = cn; ++k;
			ns += a->ns + sh.ns; nd += a->nd + sh.nd; ni += cn;
			free(ci); free_edit(&sh);
		}
		for (int s = 0; s < 2; ++s) { for (uint32_t m = 0; m < depth; ++m) free_edit(&aln[s][m]); free(aln[s]); free(cons[s]); }
		p0 += depth;
	}
	free(m0); free(s0);
	tot[0] = ns; tot[1] = nd; tot[2] = ni; tot[3] = nl;
}
"""


def edit_list(rng, counts, L_of_member, kind):
    """one of the three lists for all members: positions strictly increasing inside every member"""
    member_of = np.repeat(np.arange(len(counts)), counts)
    pos = (rng.random(len(member_of)) * (L_of_member[member_of] - 1)).astype(np.uint32)
    order = np.lexsort((pos, member_of))
    pos = pos[order]; member_of = member_of[order]
    keep = np.ones(len(pos), bool)
    keep[1:] = (pos[1:] != pos[:-1]) | (member_of[1:] != member_of[:-1])
    pos, member_of = pos[keep], member_of[keep]
    counts = np.bincount(member_of, minlength=len(counts)).astype(np.uint32)
    if kind == "subs":
        a = np.zeros(len(pos), dtype=[("pos", "u4"), ("alt", "u4")]); a["alt"] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, len(pos))]
    elif kind == "dels":
        a = np.zeros(len(pos), dtype=[("pos", "u4"), ("len", "u4")]); a["len"] = np.minimum(rng.integers(1, 21, len(pos)), L_of_member[member_of] - pos)
    else:
        a = np.zeros(len(pos), dtype=[("pos", "u4"), ("len", "u4"), ("seq_off", "u8")]); a["len"] = rng.integers(1, 21, len(pos))
        a["seq_off"] = np.cumsum(a["len"], dtype=np.uint64) - a["len"]
    a["pos"] = pos
    return a, counts


if __name__ == "__main__":
    n_edges = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    rng = np.random.default_rng(20261019)
    dll = C.CDLL(os.path.join(ROOT, "pangraph_amd", "libpgalign.so"))
    sp._bind(dll)
    n_blocks = 2 * n_edges
    lens = (L * rng.uniform(0.8, 1.2, n_blocks)).astype(np.uint32)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    cons = [letters[rng.integers(0, 4, int(n))].tobytes() for n in lens]
    B = (rc_block_t * n_blocks)()
    for b in range(n_blocks):
        B[b].consensus = cons[b]; B[b].cons_len = int(lens[b]); B[b].n_members = depth
    n_mem = n_blocks * depth
    L_of_member = np.repeat(lens, depth).astype(np.int64)
    M = np.zeros(n_mem, dtype=[("n_subs", "u4"), ("n_dels", "u4"), ("n_inss", "u4")])
    lists = {}
    for f, kind in (("n_subs", "subs"), ("n_dels", "dels"), ("n_inss", "inss")):
        lists[kind], M[f] = edit_list(rng, rng.poisson(L_of_member * 0.001 / 3).astype(np.int64), L_of_member, kind)
    S, D, I = lists["subs"], lists["dels"], lists["inss"]
    ins_seq = letters[rng.integers(0, 4, int(I["len"].sum()) + 1)].tobytes()
    E = np.zeros(n_edges, dtype=[("left", "u4"), ("right", "u4"), ("left_rc", "i4"), ("right_rc", "i4")])
    E["left"] = 2 * np.arange(n_edges); E["right"] = E["left"] + 1; E["right_rc"] = np.arange(n_edges) % 2
    P = np.concatenate([rng.permutation(depth) for _ in range(n_edges)]).astype(np.uint32)
    n_edits = len(S) + len(D) + len(I)
    args = (n_blocks, B, M.ctypes.data, S.ctypes.data, D.ctypes.data, I.ctypes.data, ins_seq, n_edges, E.ctypes.data, P.ctypes.data)
    # ---- the host loop, compiled here ----
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "host_merge.c"), "w").write(HOST_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "host_merge.c"), "-o", os.path.join(tmp, "host_merge.so")], check=True)
    host = C.CDLL(os.path.join(tmp, "host_merge.so"))
    host.host_merge.restype = None
    host.host_merge.argtypes = [C.c_int64] + [C.c_void_p] * 6 + [C.c_int64] + [C.c_void_p] * 9
    n_out = n_edges * depth
    o_cons = np.zeros(int(lens.sum()) + 1, np.uint8)
    om = np.zeros(n_out, dtype=M.dtype)
    os_, od, oi, ol = np.zeros(len(S) + 1, S.dtype), np.zeros(len(D) + 1, D.dtype), np.zeros(len(I) + 1, I.dtype), np.zeros(len(ins_seq) + 1, np.uint8)
    tot = (C.c_uint64 * 4)()
    t_dev, t_host, same = [], [], None
    for it in range(repeats + 1):                                             # the first round of both is the warm-up
        out = sp.merge_out_t()
        t0 = time.perf_counter()
        rc = dll.pga_merge_blocks(*args, C.byref(out))
        t1 = time.perf_counter()
        assert rc == 0, dll.pga_last_error()
        host.host_merge(*args, o_cons.ctypes.data, om.ctypes.data, os_.ctypes.data, od.ctypes.data, oi.ctypes.data, ol.ctypes.data, tot)
        t2 = time.perf_counter()
        if it == 0:                                                           # the two routes agree: every list as bytes, every letter
            ns, nd, ni, nl = tot[0], tot[1], tot[2], tot[3]
            dev_i = np.frombuffer(C.string_at(out.inss, ni * 16), dtype=I.dtype)
            same = (C.string_at(out.members, n_out * 12) == om.tobytes() and C.string_at(out.subs, ns * 8) == os_[:ns].tobytes() and C.string_at(out.dels, nd * 8) == od[:nd].tobytes()
                    and bool((dev_i["pos"] == oi[:ni]["pos"]).all()) and bool((dev_i["len"] == oi[:ni]["len"]).all()) and all(out.edges[e].status == 0 for e in range(n_edges)))
            base_i, base_c, at = C.addressof(out.ins_seq.contents), C.addressof(out.cons.contents), 0
            for k in rng.integers(0, ni, 20000):                                 # a sample of the insertions, letter by letter ...
                same = same and C.string_at(base_i + int(dev_i["seq_off"][k]), int(dev_i["len"][k])) == ol[int(oi["seq_off"][k]):int(oi["seq_off"][k]) + int(oi["len"][k])].tobytes()
            for e in range(n_edges):                                              # ... and every consensus
                n = out.blocks[e].cons_len
                same = same and C.string_at(C.c_void_p.from_address(C.addressof(out.blocks[e])).value, n) == o_cons[at:at + n].tobytes()
                at += n
        else:
            t_dev.append(t1 - t0); t_host.append(t2 - t1)
        dll.pga_merge_free(C.byref(out))
    med = lambda t: float(np.median(t))
    print(json.dumps(dict(edges=n_edges, depth=depth, block_len=L, output_members=n_out, edits=n_edits, consensus_letters=int(lens.sum()), repeats=repeats,
                          merge_blocks_s=dict(median=round(med(t_dev), 4), min=round(min(t_dev), 4), max=round(max(t_dev), 4)),
                          host_loop_s=dict(median=round(med(t_host), 4), min=round(min(t_host), 4), max=round(max(t_host), 4)),
                          edits_per_s=dict(merge_blocks=round(n_edits / med(t_dev)), host_loop=round(n_edits / med(t_host))),
                          identical=bool(same))))
