"""pga_plan_merge at merge scale, end to end (validation, staging, host-to-device, kernels, sorts, device-to-host: wall time of the C call
alone), with and without a resident batch, beside a plain single-threaded host loop that does the same work with the reference's structure
(reweave.rs:132-340: ids, N counts over the letters, hits sorted per block, create_intervals, refine_intervals, group_promises with
add_flanking_indel on vectors), compiled from the C++ below with g++ -O2.  The outputs are compared byte for byte.
Shapes: `leaf`: n_groups groups of two blocks of depth 1, `k` matches each that tile both blocks (hits of ~hit_len letters, gaps of 0, a few
or a few hundred letters), CIGARs of 10 .. 60 operations; `upper`: n_groups groups of eight blocks of unequal depth, k matches each between
random pairs of blocks.
usage: dev/plan_bench.py [shape=leaf] [n_groups=32] [k=1000] [hit_len=1900] [repeats=5]"""
import sys, os, time, json, subprocess, tempfile, ctypes as C
import numpy as np
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from pangraph_amd import batch, reweave as rw

HOST_CPP = r"""
#include <stdint.h>
#include <string.h>
#include <time.h>
#include <algorithm>
#include <vector>
#include "pga_align.h"
static double now(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
static uint64_t rol(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
#define P1 0x9E3779B185EBCA87ULL
#define P2 0xC2B2AE3D27D4EB4FULL
#define P3 0x165667B19E3779F9ULL
#define P4 0x85EBCA77C2B2AE63ULL
#define P5 0x27D4EB2F165667C5ULL
static uint64_t rnd(uint64_t acc, uint64_t in) { return rol(acc + in * P2, 31) * P1; }
static uint64_t xxh64_words(const uint64_t *w, int n)
{
	uint64_t h; int at = 0;
	if (n >= 4) {
		uint64_t v[4] = {P1 + P2, P2, 0, 0 - P1};
		for (; n - at >= 4; at += 4) for (int i = 0; i < 4; ++i) v[i] = rnd(v[i], w[at + i]);
		h = rol(v[0], 1) + rol(v[1], 7) + rol(v[2], 12) + rol(v[3], 18);
		for (int i = 0; i < 4; ++i) h = (h ^ rnd(0, v[i])) * P1 + P4;
	} else h = P5;
	h += (uint64_t)n * 8;
	for (; at < n; ++at) h = rol(h ^ rnd(0, w[at]), 27) * P1 + P4;
	h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
	return h;
}
static bool is_m(uint32_t k) { return k == 0 || k == 7 || k == 8; }
static void add_flanking_indel(std::vector<uint32_t> &cg, uint32_t kind, uint32_t add, bool leading)
{
	int replace = -1;
	if (leading) { for (size_t i = 0; i < cg.size(); ++i) { if (is_m(cg[i] & 15)) break; if ((cg[i] & 15) == kind) replace = (int)i; } }
	else { for (size_t i = cg.size(); i-- > 0;) { if (is_m(cg[i] & 15)) break; if ((cg[i] & 15) == kind) replace = (int)i; } }
	if (replace >= 0) cg[replace] += add << 4;
	else cg.insert(leading ? cg.begin() : cg.end(), add << 4 | kind);
}
struct Hit { uint64_t key; uint32_t side; };
/* tot: blocks with a hit, intervals, CIGAR operations, failed blocks; returns the seconds spent */
extern "C" double host_plan(int32_t n_groups, const int64_t *group_off, const pga_plan_block_t *blocks, int64_t nm, const pga_match_t *M, const uint32_t *cig, uint32_t thr,
                            pga_plan_match_t *om, pga_plan_block_res_t *ob, pga_plan_interval_t *oi, pga_slice_interval_t *osv, pga_plan_promise_t *op, uint32_t *oc, uint64_t *tot)
{
	const double t0 = now();
	const int64_t nb = group_off[n_groups];
	std::vector<uint32_t> ord((size_t)nb), idx;
	for (int32_t g = 0; g < n_groups; ++g) {
		idx.clear();
		for (int64_t b = group_off[g]; b < group_off[g + 1]; ++b) idx.push_back((uint32_t)b);
		std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return blocks[x].block_id < blocks[y].block_id; });
		for (size_t r = 0; r < idx.size(); ++r) ord[idx[r]] = (uint32_t)(group_off[g] + r);
	}
	std::vector<Hit> hits((size_t)(2 * nm));
	for (int64_t m = 0; m < nm; ++m) {
		const pga_match_t &A = M[m];
		const uint32_t rb = (uint32_t)(group_off[A.group] + A.ref), qb = (uint32_t)(group_off[A.group] + A.qry);
		const pga_plan_block_t &R = blocks[rb], &Q = blocks[qb];
		const uint64_t w[6] = {Q.block_id, (uint64_t)A.qry_start, (uint64_t)A.qry_end, R.block_id, (uint64_t)A.ref_start, (uint64_t)A.ref_end};
		pga_plan_match_t O; memset(&O, 0, sizeof(O));
		O.new_block_id = xxh64_words(w, 6);
		if (R.depth != Q.depth) O.anchor = R.depth > Q.depth ? 0 : 1;
		else {
			uint32_t rn = 0, qn = 0;
			for (int32_t i = A.ref_start; i < A.ref_end; ++i) rn += R.consensus[i] == 'N';
			for (int32_t i = A.qry_start; i < A.qry_end; ++i) qn += Q.consensus[i] == 'N';
			O.anchor = rn <= qn ? 0 : 1; O.route = 2; O.ref_n = rn; O.qry_n = qn;
		}
		om[m] = O;
		hits[2 * m] = Hit{(uint64_t)ord[rb] << 32 | (uint32_t)A.ref_start, (uint32_t)(2 * m)};
		hits[2 * m + 1] = Hit{(uint64_t)ord[qb] << 32 | (uint32_t)A.qry_start, (uint32_t)(2 * m + 1)};
	}
	std::sort(hits.begin(), hits.end(), [](const Hit &x, const Hit &y) { return x.key < y.key; });
	struct Iv { uint32_t start, end; int aligned; uint32_t side, el, er; };
	std::vector<Iv> iv; std::vector<std::pair<size_t, size_t> > mergers;
	std::vector<uint64_t> iv_of((size_t)(2 * nm)); std::vector<uint32_t> el((size_t)(2 * nm)), er((size_t)(2 * nm));
	uint64_t n_hb = 0, n_iv = 0, n_failed = 0;
	for (size_t h0 = 0; h0 < hits.size();) {
		size_t h1 = h0;
		while (h1 < hits.size() && hits[h1].key >> 32 == hits[h0].key >> 32) ++h1;
		const pga_match_t &A0 = M[hits[h0].side >> 1];
		const uint32_t b = (uint32_t)(group_off[A0.group] + ((hits[h0].side & 1) ? A0.qry : A0.ref));
		const uint32_t len = blocks[b].cons_len;
		iv.clear(); mergers.clear();
		uint32_t cursor = 0;
		for (size_t h = h0; h < h1; ++h) {                                   /* create_intervals */
			const pga_match_t &A = M[hits[h].side >> 1];
			const uint32_t s = (hits[h].side & 1) ? A.qry_start : A.ref_start, e = (hits[h].side & 1) ? A.qry_end : A.ref_end;
			if (s > cursor) iv.push_back(Iv{cursor, s, 0, 0, 0, 0});
			iv.push_back(Iv{s, e, 1, hits[h].side, 0, 0}); cursor = e;
		}
		if (cursor < len) iv.push_back(Iv{cursor, len, 0, 0, 0, 0});
		int status = 0; int64_t fail = -1;
		for (size_t n = 0; n < iv.size(); ++n) {                              /* refine_intervals */
			const uint32_t l = iv[n].end - iv[n].start;
			if (l >= thr) continue;
			const uint32_t left = n > 0 ? iv[n - 1].end - iv[n - 1].start : 0, right = n + 1 < iv.size() ? iv[n + 1].end - iv[n + 1].start : 0;
			if (iv[n].aligned) status = 1; else if (n > 0 && left < thr) status = 3; else if (n + 1 < iv.size() && right < thr) status = 5;
			if (status) { fail = (int64_t)n; break; }
			mergers.push_back(left >= right ? std::make_pair(n, n - 1) : std::make_pair(n, n + 1));
		}
		pga_plan_block_res_t B; memset(&B, 0, sizeof(B));
		B.block = b; B.status = status; B.fail_interval = fail;
		if (status) { ++n_failed; ob[n_hb++] = B; h0 = h1; continue; }
		for (size_t k = mergers.size(); k-- > 0;) {
			const size_t from = mergers[k].first, to = mergers[k].second; const uint32_t l = iv[from].end - iv[from].start;
			if (from < to) { iv[to].start = iv[from].start; iv[to].el += l; } else { iv[to].end = iv[from].end; iv[to].er += l; }
			iv.erase(iv.begin() + from);
		}
		B.first_interval = n_iv; B.n_intervals = (uint32_t)iv.size();
		ob[n_hb++] = B;
		for (size_t n = 0; n < iv.size(); ++n, ++n_iv) {
			pga_plan_interval_t I; memset(&I, 0, sizeof(I));
			I.start = iv[n].start; I.end = iv[n].end; I.aligned = iv[n].aligned; I.match = -1;
			if (iv[n].aligned) {
				const uint32_t side = iv[n].side; const int64_t m = side >> 1;
				I.new_block_id = om[m].new_block_id; I.match = m; I.is_anchor = om[m].anchor == (int32_t)(side & 1); I.reverse = M[m].reverse != 0;
				I.extend_left = iv[n].el; I.extend_right = iv[n].er;
				iv_of[side] = n_iv; el[side] = iv[n].el; er[side] = iv[n].er;
			} else { const uint64_t w[3] = {blocks[b].block_id, iv[n].start, iv[n].end}; I.new_block_id = xxh64_words(w, 3); }
			oi[n_iv] = I;
			pga_slice_interval_t S = {I.start, I.end, I.aligned && !I.is_anchor && I.reverse};
			osv[n_iv] = S;
		}
		h0 = h1;
	}
	uint64_t n_cig = 0;
	if (!n_failed) {                                                          /* group_promises */
		std::vector<uint32_t> pm((size_t)nm);
		for (int64_t m = 0; m < nm; ++m) pm[m] = (uint32_t)m;
		std::sort(pm.begin(), pm.end(), [&](uint32_t x, uint32_t y) { return M[x].group != M[y].group ? M[x].group < M[y].group : om[x].new_block_id < om[y].new_block_id; });
		std::vector<uint32_t> cg;
		for (int64_t p = 0; p < nm; ++p) {
			const uint32_t m = pm[p]; const pga_match_t &A = M[m];
			const uint32_t a = (uint32_t)om[m].anchor, q = 1 - a;
			cg.assign(cig + A.cigar_off, cig + A.cigar_off + A.n_cigar);
			if (a) {
				if (A.reverse) std::reverse(cg.begin(), cg.end());
				for (size_t i = 0; i < cg.size(); ++i) { const uint32_t k = cg[i] & 15; if (k == 1 || k == 2) cg[i] = (cg[i] & ~15u) | (3 - k); }
			}
			if (el[2 * m + a]) add_flanking_indel(cg, 2, el[2 * m + a], true);
			if (er[2 * m + a]) add_flanking_indel(cg, 2, er[2 * m + a], false);
			if (el[2 * m + q]) add_flanking_indel(cg, 1, el[2 * m + q], !A.reverse);
			if (er[2 * m + q]) add_flanking_indel(cg, 1, er[2 * m + q], A.reverse != 0);
			pga_plan_promise_t P; memset(&P, 0, sizeof(P));
			P.new_block_id = om[m].new_block_id; P.match = m; P.anchor_interval = iv_of[2 * m + a]; P.append_interval = iv_of[2 * m + q]; P.cigar_off = n_cig;
			P.anchor_block = (uint32_t)(group_off[A.group] + (a ? A.qry : A.ref)); P.append_block = (uint32_t)(group_off[A.group] + (a ? A.ref : A.qry));
			P.n_cigar = (uint32_t)cg.size(); P.reverse = A.reverse != 0;
			op[p] = P;
			memcpy(oc + n_cig, cg.data(), cg.size() * 4); n_cig += cg.size();
		}
	}
	tot[0] = n_hb; tot[1] = n_iv; tot[2] = n_cig; tot[3] = n_failed;
	return now() - t0;
}
"""


def make_level(rng, shape, n_groups, k, hit_len, thr):
    """-> (cons: per block a uint8 array, depth per block, group_off, matches as a structured array, cigars)"""
    per_group = 2 if shape == "leaf" else 8
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    M = np.zeros(n_groups * k, dtype=np.dtype([(n, t._type_) for n, t in batch.pga_match_t._fields_], align=True))
    assert M.dtype.itemsize == C.sizeof(batch.pga_match_t)
    cons, depth = [], []
    gaps = np.array([0, 0, 3, thr - 1, thr, 5 * thr, 20 * thr])
    for g in range(n_groups):
        if shape == "leaf":
            a, b = np.zeros(k, np.int64), np.ones(k, np.int64)
            depths = [1, 1]
        else:
            a = rng.integers(0, per_group, k)
            b = (a + rng.integers(1, per_group, k)) % per_group
            depths = list(rng.permutation(np.arange(1, 6 * per_group, 5))[:per_group])
        rows = M[g * k:(g + 1) * k]
        rows["group"] = g; rows["ref"] = a; rows["qry"] = b; rows["reverse"] = rng.integers(0, 2, k)
        lens = np.zeros(per_group, np.int64)
        for side, blk in (("ref", a), ("qry", b)):
            hl = rng.integers(max(thr, hit_len // 2), hit_len * 3 // 2 + 1, k)
            gp = gaps[rng.integers(0, len(gaps), k)]
            start = np.zeros(k, np.int64)
            order = rng.permutation(k) if side == "qry" else np.arange(k)       # the hits of the qry side lie in another order
            for j in order:
                start[j] = lens[blk[j]] + gp[j]
                lens[blk[j]] = start[j] + hl[j]
            rows[side + "_start"] = start; rows[side + "_end"] = start + hl
        for j in range(per_group):
            cons.append(letters[rng.integers(0, 4, int(lens[j]) + int(gaps[rng.integers(0, len(gaps))]) + 1)])
            depth.append(int(depths[j]))
    n_cig = rng.integers(10, 61, len(M))
    M["n_cigar"] = n_cig
    M["cigar_off"] = np.cumsum(n_cig) - n_cig
    kinds = np.array([0, 0, 0, 1, 2, 7, 8], np.uint32)
    cig = (rng.integers(1, 200, int(n_cig.sum())).astype(np.uint32) << 4) | kinds[rng.integers(0, len(kinds), int(n_cig.sum()))]
    first = M["cigar_off"].astype(np.int64)
    cig[first] = (cig[first] & ~np.uint32(15)) | np.array([0, 1, 2], np.uint32)[rng.integers(0, 3, len(M))]          # a leading indel now and then
    return cons, depth, [per_group * g for g in range(n_groups + 1)], M, cig


if __name__ == "__main__":
    shape = sys.argv[1] if len(sys.argv) > 1 else "leaf"
    n_groups = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 1000
    hit_len = int(sys.argv[4]) if len(sys.argv) > 4 else 1900
    repeats = int(sys.argv[5]) if len(sys.argv) > 5 else 5
    thr = 100
    rng = np.random.default_rng(20261019)
    dll = batch.lib()
    rw._bind(dll)
    cons, depth, off, M, cig = make_level(rng, shape, n_groups, k, hit_len, thr)
    nb, nm = len(cons), len(M)
    B = (rw.plan_block_t * nb)()
    for i, c in enumerate(cons):
        B[i].block_id = int(rng.integers(1, 1 << 62)); B[i].cons_len = len(c); B[i].depth = depth[i]
        C.c_void_p.from_address(C.addressof(B[i]) + rw.plan_block_t.consensus.offset).value = c.ctypes.data
    goff = (C.c_int64 * len(off))(*off)
    args = (n_groups, goff, B, nm, M.ctypes.data, cig.ctypes.data, len(cig))
    groups = [cons[off[g]:off[g + 1]] for g in range(n_groups)]
    rb = batch.ResidentBatch(batch.PreparedBatch(groups))
    seq_index = (C.c_int64 * nb)(*range(nb))
    # ---- the host loop, compiled here ----
    tmp = tempfile.mkdtemp()
    open(os.path.join(tmp, "host_plan.cpp"), "w").write(HOST_CPP)
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), os.path.join(tmp, "host_plan.cpp"), "-o", os.path.join(tmp, "host_plan.so")], check=True)
    host = C.CDLL(os.path.join(tmp, "host_plan.so"))
    host.host_plan.restype = C.c_double
    host.host_plan.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 7
    cap_iv, cap_cig = 4 * nm + nb, len(cig) + 4 * nm
    h_m, h_b = (rw.plan_match_t * nm)(), (rw.plan_block_res_t * nb)()
    h_i, h_s = (rw.plan_interval_t * cap_iv)(), (rw.slice_interval_t * cap_iv)()
    h_p, h_c, tot = (rw.plan_promise_t * nm)(), (C.c_uint32 * cap_cig)(), (C.c_uint64 * 4)()
    t_dev, t_res, t_host, same, routes = [], [], [], None, None
    for it in range(repeats + 1):                                             # the first round of each is the warm-up
        out, res = rw.plan_out_t(), rw.plan_out_t()
        t0 = time.perf_counter()
        rc = dll.pga_plan_merge(*args, thr, None, None, C.byref(out))
        t1 = time.perf_counter()
        assert rc == 0, dll.pga_last_error()
        rc = dll.pga_plan_merge(*args, thr, rb.h, seq_index, C.byref(res))
        t2 = time.perf_counter()
        assert rc == 0, dll.pga_last_error()
        secs = host.host_plan(n_groups, goff, B, nm, M.ctypes.data, cig.ctypes.data, thr, h_m, h_b, h_i, h_s, h_p, h_c, tot)
        if it == 0:
            n_hb, n_iv, n_cg, n_failed = tot[0], tot[1], tot[2], tot[3]
            S = lambda p, n, t: C.string_at(p, n * C.sizeof(t))
            same = (out.n_failed == res.n_failed == n_failed == 0 and out.n_blocks == n_hb and out.n_intervals == res.n_intervals == n_iv and out.n_cigar == res.n_cigar == n_cg
                    and S(out.matches, nm, rw.plan_match_t) == S(h_m, nm, rw.plan_match_t) and S(out.blocks, n_hb, rw.plan_block_res_t) == S(h_b, n_hb, rw.plan_block_res_t)
                    and all(S(o.intervals, n_iv, rw.plan_interval_t) == S(h_i, n_iv, rw.plan_interval_t) and S(o.slice_intervals, n_iv, rw.slice_interval_t) == S(h_s, n_iv, rw.slice_interval_t)
                            and S(o.promises, nm, rw.plan_promise_t) == S(h_p, nm, rw.plan_promise_t) and S(o.cigars, n_cg, C.c_uint32) == S(h_c, n_cg, C.c_uint32) for o in (out, res))
                    and all(res.matches[m].anchor == h_m[m].anchor for m in range(0, nm, max(nm // 1000, 1))))
            routes = dict(without_batch=[out.counters.by_depth, out.counters.by_mask, out.counters.by_letters], with_batch=[res.counters.by_depth, res.counters.by_mask, res.counters.by_letters])
            sizes = dict(intervals_before=out.counters.intervals_before, intervals_after=out.counters.intervals_after, cigar_in=out.counters.cigar_in, cigar_out=out.counters.cigar_out)
        else:
            t_dev.append(t1 - t0); t_res.append(t2 - t1); t_host.append(secs)
        dll.pga_plan_free(C.byref(out)); dll.pga_plan_free(C.byref(res))
    rb.close()
    stat = lambda t: dict(median=round(float(np.median(t)), 5), min=round(min(t), 5), max=round(max(t), 5))
    print(json.dumps(dict(shape=shape, groups=n_groups, blocks=nb, matches=nm, letters=int(sum(len(c) for c in cons)), repeats=repeats, routes=routes, **sizes,
                          plan_merge_s=stat(t_dev), plan_merge_with_batch_s=stat(t_res), host_loop_s=stat(t_host), identical=bool(same))))
