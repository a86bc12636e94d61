"""pga_detach_unaligned at merge scale, end to end (validation, host-to-device, kernels, device-to-host, the block ids: wall time of the C
call alone), beside a plain single-threaded host loop with the reference's structure (detach_unaligned.rs:24-114: per block every member's
aligned_count, the unaligned ones removed, Edit::apply on a clone of the consensus -- substitutions, '-' over every deletion, the sorted
insertions spliced in back to front, the '-' stripped --, reverse_complement, XXH64 for the block id), compiled from the C below with gcc -O2.
The reference leaves the kept members where they are; this entry hands them out packed, so the host loop is timed in two parts: what the
reference does, and the packing of the kept lists that makes its output comparable.
Shape: n_blocks blocks of block_len letters (+-20 %), `depth` members each, ~0.1 % edits per member (a third each substitutions, deletions
of 1..20, insertions of 1..20, lists sorted by position); `share` of the members are unaligned: one deletion over the whole consensus and one
insertion of about block_len letters; every second of them is reverse.
usage: dev/detach_bench.py [n_blocks=1000] [depth=500] [block_len=10000] [repeats=5] [share=0.01]"""
import sys, os, time, json, subprocess, tempfile, ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pangraph_amd import detach as dt
from pangraph_amd.reconsensus import rc_block_t
from simplify_bench import edit_list

HOST_C = r"""
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "pga_align.h"
static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static char comp(char c) { switch (c) { case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A'; default: return c; } }
static uint64_t rol(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
static uint64_t rd64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
#define P1 0x9E3779B185EBCA87ULL
#define P2 0xC2B2AE3D27D4EB4FULL
#define P3 0x165667B19E3779F9ULL
#define P4 0x85EBCA77C2B2AE63ULL
#define P5 0x27D4EB2F165667C5ULL
static uint64_t rnd(uint64_t acc, uint64_t in) { return rol(acc + in * P2, 31) * P1; }
static uint64_t xxh64(const uint8_t *p, uint64_t n)
{
	const uint8_t *end = p + n; uint64_t h;
	if (n >= 32) {
		uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
		for (; end - p >= 32; p += 32) for (int i = 0; i < 4; ++i) v[i] = rnd(v[i], rd64(p + 8 * i));
		h = rol(v[0], 1) + rol(v[1], 7) + rol(v[2], 12) + rol(v[3], 18);
		for (int i = 0; i < 4; ++i) h = (h ^ rnd(0, v[i])) * P1 + P4;
	} else h = P5;
	h += n;
	for (; end - p >= 8; p += 8) h = rol(h ^ rnd(0, rd64(p)), 27) * P1 + P4;
	if (end - p >= 4) { uint32_t w; memcpy(&w, p, 4); h = rol(h ^ (w * P1), 23) * P2 + P3; p += 4; }
	for (; p < end; ++p) h = rol(h ^ (*p * P5), 11) * P1;
	h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
	return h;
}
static const char *g_seq;
static int by_pos_seq(const void *a, const void *b)
{
	const pga_ins_t *x = (const pga_ins_t*)a, *y = (const pga_ins_t*)b;
	if (x->pos != y->pos) return x->pos < y->pos ? -1 : 1;
	const uint32_t n = x->len < y->len ? x->len : y->len; const int c = memcmp(g_seq + x->seq_off, g_seq + y->seq_off, n);
	return c ? c : (x->len < y->len ? -1 : x->len > y->len);
}
/* secs[2]: the reference's work, the packing of the kept lists; o_letters: the orphans' sequences one after the other */
void host_detach(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *mem, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq,
                 const pga_detach_member_t *who, uint32_t *o_kept, pga_rc_member_t *om, pga_sub_t *os, pga_del_t *od, pga_ins_t *oi, int64_t *map, pga_detach_orphan_t *orph,
                 char *o_letters, uint64_t *tot, double *secs)
{
	const double t0 = now();
	uint64_t n_mem = 0;
	for (int64_t b = 0; b < n_blocks; ++b) n_mem += blocks[b].n_members;
	uint64_t *s0 = (uint64_t*)malloc((n_mem + 1) * 3 * sizeof(uint64_t)), *d0 = s0 + n_mem + 1, *i0 = d0 + n_mem + 1;
	s0[0] = d0[0] = i0[0] = 0;
	for (uint64_t m = 0; m < n_mem; ++m) { s0[m + 1] = s0[m] + mem[m].n_subs; d0[m + 1] = d0[m] + mem[m].n_dels; i0[m + 1] = i0[m] + mem[m].n_inss; }
	uint8_t *un = (uint8_t*)calloc(n_mem + 1, 1);
	uint64_t m = 0, n_orph = 0, nl = 0;
	g_seq = ins_seq;
	for (int64_t b = 0; b < n_blocks; ++b) {                               /* extract_unaligned_nodes, block after block */
		const uint32_t L = blocks[b].cons_len;
		o_kept[b] = 0;
		for (uint32_t k = 0; k < blocks[b].n_members; ++k, ++m) {
			uint64_t sum = 0;
			for (uint64_t t = d0[m]; t < d0[m + 1]; ++t) sum += dels[t].len;
			if (sum < L) { ++o_kept[b]; continue; }
			un[m] = 1;
			/* Edit::apply on a clone of the consensus */
			uint64_t cap = L, len = L;
			for (uint64_t t = i0[m]; t < i0[m + 1]; ++t) cap += inss[t].len;
			char *q = (char*)malloc(cap + 1); memcpy(q, blocks[b].consensus, L);
			for (uint64_t t = s0[m]; t < s0[m + 1]; ++t) q[subs[t].pos] = (char)subs[t].alt;
			for (uint64_t t = d0[m]; t < d0[m + 1]; ++t) memset(q + dels[t].pos, '-', dels[t].len);
			const uint32_t ni = mem[m].n_inss;
			pga_ins_t *srt = (pga_ins_t*)malloc((ni + 1) * sizeof(pga_ins_t)); memcpy(srt, inss + i0[m], ni * sizeof(pga_ins_t));
			qsort(srt, ni, sizeof(pga_ins_t), by_pos_seq);
			for (uint32_t t = ni; t-- > 0;) { memmove(q + srt[t].pos + srt[t].len, q + srt[t].pos, len - srt[t].pos); memcpy(q + srt[t].pos, ins_seq + srt[t].seq_off, srt[t].len); len += srt[t].len; }
			uint64_t w = 0;
			for (uint64_t r = 0; r < len; ++r) if (q[r] != '-') q[w++] = q[r];
			if (who[m].reverse) { for (uint64_t i = 0; i < w / 2; ++i) { char a = comp(q[i]); q[i] = comp(q[w - 1 - i]); q[w - 1 - i] = a; } if (w & 1) q[w / 2] = comp(q[w / 2]); }
			uint8_t *msg = (uint8_t*)malloc(16 + w);                          /* (node_id, &seq).hash() */
			const uint64_t nid = who[m].node_id; memcpy(msg, &nid, 8); memcpy(msg + 8, &w, 8); memcpy(msg + 16, q, w);
			pga_detach_orphan_t O; memset(&O, 0, sizeof(O));
			O.member = m; O.node_id = nid; O.block_id = xxh64(msg, 16 + w); O.block = (uint32_t)(n_blocks + n_orph); O.len = (uint32_t)w;
			orph[n_orph++] = O;
			memcpy(o_letters + nl, q, w); nl += w;
			free(msg); free(srt); free(q);
		}
	}
	const double t1 = now();
	uint64_t k = 0, ns = 0, nd = 0, ni = 0, n_kept = n_mem - n_orph, r = 0;
	for (m = 0; m < n_mem; ++m) {
		if (un[m]) { map[m] = (int64_t)(n_kept + r); memset(&om[n_kept + r], 0, sizeof(om[0])); ++r; continue; }
		memcpy(os + ns, subs + s0[m], mem[m].n_subs * sizeof(pga_sub_t)); memcpy(od + nd, dels + d0[m], mem[m].n_dels * sizeof(pga_del_t)); memcpy(oi + ni, inss + i0[m], mem[m].n_inss * sizeof(pga_ins_t));
		ns += mem[m].n_subs; nd += mem[m].n_dels; ni += mem[m].n_inss;
		map[m] = (int64_t)k; om[k++] = mem[m];
	}
	free(un); free(s0);
	tot[0] = ns; tot[1] = nd; tot[2] = ni; tot[3] = n_orph; tot[4] = nl;
	secs[0] = t1 - t0; secs[1] = now() - t1;
}
"""


def add_orphans(a, counts, at_members, entries):
    """one more entry for each of at_members (whose count is 0) in a packed list"""
    first = np.cumsum(counts) - counts
    a = np.insert(a, first[at_members], entries)
    counts = counts.copy(); counts[at_members] = 1
    return a, counts


if __name__ == "__main__":
    n_blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    depth = int(sys.argv[2]) if len(sys.argv) > 2 else 500
    L = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
    repeats = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    share = float(sys.argv[5]) if len(sys.argv) > 5 else 0.01
    rng = np.random.default_rng(20261019)
    dll = C.CDLL(os.path.join(ROOT, "pangraph_amd", "libpgalign.so"))
    dt._bind(dll)
    lens = (L * rng.uniform(0.8, 1.2, n_blocks)).astype(np.uint32)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    cons = [letters[rng.integers(0, 4, int(n))].tobytes() for n in lens]
    B = (rc_block_t * n_blocks)()
    for b in range(n_blocks):
        B[b].consensus = cons[b]; B[b].cons_len = int(lens[b]); B[b].n_members = depth
    n_mem = n_blocks * depth
    L_of_member = np.repeat(lens, depth).astype(np.int64)
    orphans = np.sort(rng.choice(n_mem, max(int(n_mem * share), 1), replace=False))
    M = np.zeros(n_mem, dtype=[("n_subs", "u4"), ("n_dels", "u4"), ("n_inss", "u4")])
    lists = {}
    for f, kind in (("n_subs", "subs"), ("n_dels", "dels"), ("n_inss", "inss")):
        want = rng.poisson(L_of_member * 0.001 / 3).astype(np.int64)
        want[orphans] = 0
        lists[kind], M[f] = edit_list(rng, want, L_of_member, kind)
    D_o = np.zeros(len(orphans), lists["dels"].dtype); D_o["len"] = L_of_member[orphans]
    I_o = np.zeros(len(orphans), lists["inss"].dtype); I_o["len"] = (L_of_member[orphans] * rng.uniform(0.8, 1.2, len(orphans))).astype(np.uint32)
    lists["dels"], M["n_dels"] = add_orphans(lists["dels"], M["n_dels"].astype(np.int64), orphans, D_o)
    lists["inss"], M["n_inss"] = add_orphans(lists["inss"], M["n_inss"].astype(np.int64), orphans, I_o)
    S, D, I = lists["subs"], lists["dels"], lists["inss"]
    I["seq_off"] = np.cumsum(I["len"], dtype=np.uint64) - I["len"]
    ins_seq = letters[rng.integers(0, 4, int(I["len"].sum()) + 1)].tobytes()
    W = np.zeros(n_mem, dtype=[("node_id", "u8"), ("reverse", "i4"), ("pad", "i4")])
    W["node_id"] = rng.integers(1, 1 << 62, n_mem, dtype=np.uint64); W["reverse"][orphans[::2]] = 1
    n_edits = len(S) + len(D) + len(I)
    args = (n_blocks, B, M.ctypes.data, S.ctypes.data, D.ctypes.data, I.ctypes.data, ins_seq, W.ctypes.data)
    # ---- the host loop, compiled here ----
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "host_detach.c"), "w").write(HOST_C)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "host_detach.c"), "-o", os.path.join(tmp, "host_detach.so")], check=True)
    host = C.CDLL(os.path.join(tmp, "host_detach.so"))
    host.host_detach.restype = None
    host.host_detach.argtypes = [C.c_int64] + [C.c_void_p] * 17
    o_kept = np.zeros(n_blocks, np.uint32)
    om = np.zeros(n_mem, M.dtype)
    os_, od, oi = np.zeros(len(S) + 1, S.dtype), np.zeros(len(D) + 1, D.dtype), np.zeros(len(I) + 1, I.dtype)
    omap = np.zeros(n_mem, np.int64)
    O = np.zeros(len(orphans) + 1, dtype=[("member", "u8"), ("node_id", "u8"), ("block_id", "u8"), ("block", "u4"), ("len", "u4"), ("status", "i4"), ("pad", "i4")])
    ol = np.zeros(int(I_o["len"].sum()) + 1, np.uint8)
    tot = (C.c_uint64 * 5)(); secs = (C.c_double * 2)()
    t_dev, t_host, t_host_ref, same = [], [], [], None
    for it in range(repeats + 1):                                             # the first round of both is the warm-up
        out = dt.detach_out_t()
        t0 = time.perf_counter()
        rc = dll.pga_detach_unaligned(*args, C.byref(out))
        t1 = time.perf_counter()
        assert rc == 0, dll.pga_last_error()
        host.host_detach(*args, o_kept.ctypes.data, om.ctypes.data, os_.ctypes.data, od.ctypes.data, oi.ctypes.data, omap.ctypes.data, O.ctypes.data, ol.ctypes.data, tot, secs)
        t2 = time.perf_counter()
        if it == 0:                                                           # the two routes agree: every list as bytes, every orphan record, every letter
            ns, nd, ni, no = tot[0], tot[1], tot[2], tot[3]
            same = (out.n_orphans == no == len(orphans) and out.n_blocks == n_blocks + no and C.string_at(out.members, n_mem * 12) == om.tobytes()
                    and C.string_at(out.subs, ns * 8) == os_[:ns].tobytes() and C.string_at(out.dels, nd * 8) == od[:nd].tobytes() and C.string_at(out.inss, ni * 16) == oi[:ni].tobytes()
                    and C.string_at(out.member_map, n_mem * 8) == omap.tobytes() and C.string_at(out.orphans, no * O.dtype.itemsize) == O[:no].tobytes()
                    and all(out.blocks[b].n_members == o_kept[b] for b in range(n_blocks)))
            at = 0
            for k in range(no):
                blk = out.blocks[n_blocks + k]
                same = same and blk.n_members == 1 and blk.cons_len == O["len"][k] and C.string_at(C.c_void_p.from_address(C.addressof(blk)).value, blk.cons_len) == ol[at:at + blk.cons_len].tobytes()
                at += blk.cons_len
        else:
            t_dev.append(t1 - t0); t_host.append(secs[0] + secs[1]); t_host_ref.append(secs[0])
        dll.pga_detach_free(C.byref(out))
    med = lambda t: float(np.median(t))
    print(json.dumps(dict(blocks=n_blocks, depth=depth, block_len=L, members=n_mem, orphans=len(orphans), orphan_letters=int(I_o["len"].sum()), edits=n_edits, repeats=repeats,
                          detach_unaligned_s=dict(median=round(med(t_dev), 4), min=round(min(t_dev), 4), max=round(max(t_dev), 4)),
                          host_loop_s=dict(median=round(med(t_host), 4), min=round(min(t_host), 4), max=round(max(t_host), 4)),
                          host_loop_without_packing_s=dict(median=round(med(t_host_ref), 4), min=round(min(t_host_ref), 4), max=round(max(t_host_ref), 4)),
                          identical=bool(same))))
