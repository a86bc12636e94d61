// pga_promise.hip -- SURVEY 8(f)-1, the whole of MergePromise::solve_promise (packages/pangraph/src/pangraph/reweave.rs:40-94) for all
// promises of a merge: consensus sequences, edit lists, CIGARs and orientations in, every member's edits against its anchor consensus out.
//   edits.rs:538-566                  Edit::from_cigar, then BandParameters::from_edits over the anchor (once per promise)
//   edits.rs:307-329                  Edit::apply of every member's edits to the append consensus
//   io/seq.rs:9-33                    reverse_complement of the member sequence on a reverse promise
//   edits.rs:29-34, 68-73, 99-104, 257-276   Edit::reverse_complement (positions mirrored, every list stably sorted) for the member's band
//   align/map_variations.rs:23-37     the two bands summed, then map_variations (pga_mapvar.hip)
// What runs where:
//   host     list bookkeeping over the edit lists, O(number of edits): validation, the list-order rules of Edit::apply (prepare_edit), the
//            band arithmetic (pga_edits.h) and a SEGMENT TABLE per member: the member's sequence as a chain of runs, each either a stretch
//            of the append consensus, the letters of one insertion, or the single letter of a substitution (a substitution cuts the run
//            it lies in, so that no thread has to search the substitutions letter by letter; the last of equal positions wins and a
//            deleted position never starts a run, both decided here)
//   device   k_promise_build writes every member sequence, oriented, into the ASCII buffer the aligner reads (the letters never reach
//            the host); the alignment itself (k_mapvar*)
// Promises are processed in chunks whose built sequences stay under PGA_PROMISE_CHUNK_MB (default 2048; a single promise larger than that
// is a chunk of its own); results are packed per member in input order, so the output does not depend on the chunking.
#include "pga_common.h"
#include "../../include/pga_align.h"
#include "pga_runs.h"
#include <unordered_map>

namespace pga {

struct MvDevJob { uint64_t ref_off, qry_off; uint32_t ref_len, qry_len; int32_t mean_shift; uint32_t band_width; };
void map_variations_dev(int64_t n, const MvDevJob *jobs, const char *d_ascii, uint64_t cat_size, const pga_mapvar_params_t &prm, pga_mapvar_res_t *res,
                        std::vector<pga_sub_t> &h_subs, std::vector<pga_del_t> &h_dels, std::vector<pga_ins_t> &h_inss, std::vector<char> &h_seq, hipStream_t st);

// (the complement table, PrSeg -- one run of a member sequence -- and promise_segments: pga_runs.h)
// dst: offset of the sequence in the ASCII buffer (a multiple of 4: a thread stores four letters at once); word0: the first of its words
// among all words of the launch
struct PrJob { uint64_t dst, seg_off, word0; uint32_t n_seg, len, reverse, pad; };

constexpr int PR_THREADS = 256, PR_LETTERS = 4;           // a workgroup writes a tile of 1024 letters

// One thread per four WRITTEN letters i .. i+3 of a job.  Written letter i is built letter i of a forward job and the complement of
// built letter len-1-i of a reverse job (the mirrored index is on the load side, so that the store is one aligned word either way).
__global__ __launch_bounds__(PR_THREADS) void k_promise_build(const PrJob *__restrict__ jobs, int n_jobs, uint64_t n_words, const PrSeg *__restrict__ segs,
                                                              const char *__restrict__ cons, const char *__restrict__ ins_seq, char *__restrict__ out, uint32_t *__restrict__ rejected)
{
	__shared__ uint8_t s_comp[256];
	s_comp[threadIdx.x] = d_comp.t[threadIdx.x];
	__syncthreads();
	for (uint64_t w = (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x; w < n_words; w += (uint64_t)gridDim.x * PR_THREADS) {
		int lo = 0, hi = n_jobs - 1;                                        // the last job with word0 <= w (jobs have at least one word)
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].word0 <= w) lo = mid; else hi = mid - 1; }
		const PrJob J = jobs[lo];
		const uint32_t i0 = (uint32_t)(w - J.word0) * PR_LETTERS;
		const PrSeg *S = segs + J.seg_off;
		uint32_t s_beg = 1, s_end = 0, kind = 0; uint64_t src = 0;          // the run the previous letter came from (none yet)
		uint32_t word = 0; bool bad = false;
#pragma unroll
		for (int k = 0; k < PR_LETTERS; ++k) {
			const uint32_t i = i0 + (uint32_t)k;
			if (i >= J.len) break;
			const uint32_t b = J.reverse ? J.len - 1 - i : i;
			if (b < s_beg || b >= s_end) {
				uint32_t a = 0, z = J.n_seg - 1;                                // the last run with out <= b
				while (a < z) { const uint32_t mid = (a + z + 1) >> 1; if (S[mid].out <= b) a = mid; else z = mid - 1; }
				const PrSeg g = S[a];
				s_beg = g.out; kind = g.kind; src = g.src;
				s_end = a + 1 < J.n_seg ? S[a + 1].out : J.len;
			}
			uint32_t c = kind == 0 ? (uint8_t)cons[src + (b - s_beg)] : kind == 1 ? (uint8_t)ins_seq[src + (b - s_beg)] : (uint32_t)(src & 255u);
			if (J.reverse) { const uint32_t cc = s_comp[c]; if (cc) c = cc; else bad = true; }
			word |= c << (8 * k);
		}
		*reinterpret_cast<uint32_t*>(out + J.dst + i0) = word;
		if (bad) atomicOr(&rejected[lo], 1u);
	}
}

// ---------------------------------------------------------------- host side
struct PromiseStage { int32_t *status, *mean_shift; uint32_t *band_width; uint64_t *seq_off; std::vector<char> seqs; };

// what the host works out for one member before anything runs on the device
struct PrMember { int32_t status; uint32_t len; int64_t ms, bw; std::vector<PrSeg> segs; };

static size_t promise_chunk_bytes()
{
	const char *e = getenv("PGA_PROMISE_CHUNK_MB");
	const double mb = e ? atof(e) : 2048.0;
	return (size_t)(std::max(mb, 1.0) * (double)(1u << 20));
}

void solve_promises_host(int64_t n_promises, const pga_promise_t *promises, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                         const char *ins_seq, const pga_mapvar_params_t &prm, pga_mapvar_res_t *res, std::vector<pga_sub_t> &o_subs, std::vector<pga_del_t> &o_dels,
                         std::vector<pga_ins_t> &o_inss, std::vector<char> &o_iseq, PromiseStage *stage)
{
	hipStream_t st = 0;
	const char *who = stage ? "pga_stage_promise_jobs" : "pga_solve_promises";
	auto fail = [&](const std::string &what) { throw std::runtime_error(std::string(who) + ": " + what); };
	// ---- offsets, validation, the cigar band of every promise ----
	std::vector<uint64_t> mem_first((size_t)n_promises + 1, 0);
	for (int64_t p = 0; p < n_promises; ++p) mem_first[p + 1] = mem_first[p] + promises[p].n_members;
	const uint64_t n_mem = mem_first[n_promises];
	if (n_mem && !members) fail("null member list");
	std::vector<uint64_t> sub_off(n_mem + 1, 0), del_off(n_mem + 1, 0), ins_off(n_mem + 1, 0);
	for (uint64_t m = 0; m < n_mem; ++m) { sub_off[m + 1] = sub_off[m] + members[m].n_subs; del_off[m + 1] = del_off[m] + members[m].n_dels; ins_off[m + 1] = ins_off[m] + members[m].n_inss; }
	if ((sub_off[n_mem] && !subs) || (del_off[n_mem] && !dels) || (ins_off[n_mem] && !inss)) fail("null edit list");
	struct CigarBand { bool ok; int64_t ms, bw; };
	std::vector<CigarBand> cband((size_t)n_promises);
	for (int64_t p = 0; p < n_promises; ++p) {
		const pga_promise_t &Q = promises[p];
		if ((Q.anchor_len && !Q.anchor) || (Q.append_len && !Q.append)) fail("null consensus with a non-zero length (promise " + std::to_string(p) + ")");
		if (Q.anchor_len >= (1u << 30) || Q.append_len >= (1u << 30)) fail("consensus longer than 2^30");
		if (Q.n_cigar && !Q.cigar) fail("null cigar with a non-zero length (promise " + std::to_string(p) + ")");
		std::vector<pga_del_t> cd; std::vector<std::pair<uint32_t, uint32_t>> ci;
		uint64_t rpos = 0;
		for (uint32_t t = 0; t < Q.n_cigar; ++t) {                           // Edit::from_cigar (edits.rs:538-566)
			const uint32_t op = Q.cigar[t] & 15u, len = Q.cigar[t] >> 4;
			if (op == 0 || op == 7 || op == 8) rpos += len;
			else if (op == 1) ci.emplace_back((uint32_t)rpos, len);
			else if (op == 2) { cd.push_back(pga_del_t{(uint32_t)rpos, len}); rpos += len; }
			else fail(std::string("unsupported CIGAR operation '") + "MIDNSHP=XB??????"[op] + "' (promise " + std::to_string(p) + ")");
			if (rpos >= (1ULL << 31)) fail("cigar spans more than 2^31 reference positions");
		}
		cband[p].ok = band_from_edits(cd, ci, Q.anchor_len, cband[p].ms, cband[p].bw);
		for (uint64_t m = mem_first[p]; m < mem_first[p + 1]; ++m) {
			for (uint64_t t = sub_off[m]; t < sub_off[m + 1]; ++t) if (subs[t].pos >= Q.append_len) fail("substitution beyond the append consensus (member " + std::to_string(m) + ")");
			for (uint64_t t = del_off[m]; t < del_off[m + 1]; ++t) if ((uint64_t)dels[t].pos + dels[t].len > Q.append_len) fail("deletion beyond the append consensus (member " + std::to_string(m) + ")");
			for (uint64_t t = ins_off[m]; t < ins_off[m + 1]; ++t) {
				if (inss[t].pos > Q.append_len) fail("insertion beyond the append consensus (member " + std::to_string(m) + ")");
				if (inss[t].len && !ins_seq) fail("null insertion letters with a non-zero length (member " + std::to_string(m) + ")");
			}
		}
	}
	if (stage) stage->seq_off[0] = 0;
	o_subs.clear(); o_dels.clear(); o_inss.clear(); o_iseq.clear();
	const size_t chunk_cap = promise_chunk_bytes();
	const int n_threads = range_threads();
	std::vector<PrMember> pm;
	int64_t p0 = 0;
	while (p0 < n_promises) {
		// ---- the chunk: promises p0 .. p1 (an upper bound of a member's length: consensus + inserted letters) ----
		int64_t p1 = p0; size_t bound = 0;
		while (p1 < n_promises) {
			size_t b = 0;
			for (uint64_t m = mem_first[p1]; m < mem_first[p1 + 1]; ++m) { b += (size_t)promises[p1].append_len + 4; for (uint64_t t = ins_off[m]; t < ins_off[m + 1]; ++t) b += inss[t].len; }
			if (p1 > p0 && bound + b > chunk_cap) break;
			bound += b; ++p1;
		}
		const uint64_t m0 = mem_first[p0], m1 = mem_first[p1];
		// the slice of the insertion letters the chunk reads, and one copy of every distinct consensus
		uint64_t il = UINT64_MAX, ih = 0;
		for (uint64_t t = ins_off[m0]; t < ins_off[m1]; ++t) if (inss[t].len) { il = std::min<uint64_t>(il, inss[t].seq_off); ih = std::max<uint64_t>(ih, inss[t].seq_off + inss[t].len); }
		if (il > ih) il = ih = 0;
		struct Placed { uint32_t len; uint64_t off; };
		std::unordered_map<const char*, Placed> seen_anchor, seen_append;
		std::vector<char> h_anchor, h_append;
		auto place = [](std::unordered_map<const char*, Placed> &seen, std::vector<char> &cat, const char *s, uint32_t len) -> uint64_t {
			auto it = seen.find(s);
			if (it != seen.end() && it->second.len == len) return it->second.off;
			const uint64_t off = cat.size();
			cat.insert(cat.end(), s, s + len);
			seen[s] = Placed{len, off};
			return off;
		};
		std::vector<uint64_t> anchor_at((size_t)(p1 - p0)), append_at((size_t)(p1 - p0));
		for (int64_t p = p0; p < p1; ++p) { anchor_at[p - p0] = place(seen_anchor, h_anchor, promises[p].anchor, promises[p].anchor_len); append_at[p - p0] = place(seen_append, h_append, promises[p].append, promises[p].append_len); }
		// ---- per member: status before alignment, band, segment table (a few host threads, members are independent) ----
		pm.clear(); pm.resize((size_t)(m1 - m0));
		std::vector<uint32_t> promise_of((size_t)(m1 - m0));
		for (int64_t p = p0; p < p1; ++p) for (uint64_t m = mem_first[p]; m < mem_first[p + 1]; ++m) promise_of[m - m0] = (uint32_t)(p - p0);
		auto work = [&](uint64_t a, uint64_t z) {
			PreparedEdit P; std::vector<pga_del_t> dl; std::vector<std::pair<uint32_t, uint32_t>> ml;
			for (uint64_t m = a; m < z; ++m) {
				PrMember &M = pm[m - m0];
				const int64_t p = p0 + promise_of[m - m0];
				const pga_promise_t &Q = promises[p];
				M.status = 0; M.len = 0; M.ms = M.bw = 0;
				if (!cband[p].ok) { M.status = 8; continue; }                     // reweave.rs:47: the reference fails before its loop
				const pga_sub_t *ms_ = subs + sub_off[m]; const pga_del_t *md = dels + del_off[m]; const pga_ins_t *mi = inss + ins_off[m];
				const uint32_t ns = members[m].n_subs, nd = members[m].n_dels, ni = members[m].n_inss;
				prepare_edit(ms_, ns, md, nd, mi, ni, ins_seq, Q.append_len, P);
				M.len = promise_segments(P, Q.append_len, append_at[p - p0], il, M.segs);
				if (M.len == 0) continue;                                         // reweave.rs:56-57: Edit::deleted(anchor_len), not aligned
				dl.assign(md, md + nd); ml.clear();
				for (uint32_t t = 0; t < ni; ++t) ml.emplace_back(mi[t].pos, mi[t].len);
				if (Q.reverse) {
					// a letter the complement table rejects, in an edit (Sub / Ins::reverse_complement); the built sequence is checked by the kernel
					bool bad = false;
					for (uint32_t t = 0; t < ns && !bad; ++t) bad = ms_[t].alt > 255u || !h_comp.t[ms_[t].alt];
					for (uint32_t t = 0; t < ni && !bad; ++t) for (uint32_t c = 0; c < mi[t].len && !bad; ++c) bad = !h_comp.t[(uint8_t)ins_seq[mi[t].seq_off + c]];
					if (bad) { M.status = 9; continue; }
					for (pga_del_t &d : dl) d.pos = Q.append_len - d.pos - d.len;   // edits.rs:68-73, then sort_by_key (stable)
					std::stable_sort(dl.begin(), dl.end(), [](const pga_del_t &x, const pga_del_t &y) { return x.pos < y.pos; });
					for (auto &x : ml) x.first = Q.append_len - x.first;            // edits.rs:99-104
					std::stable_sort(ml.begin(), ml.end(), [](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return x.first < y.first; });
				}
				int64_t ms = 0, bw = 0;
				if (!band_from_edits(dl, ml, Q.append_len, ms, bw)) { M.status = 7; continue; }   // map_variations.rs:29-37 (checked after the sequence: status 9 wins)
				M.ms = ms + cband[p].ms; M.bw = bw + cband[p].bw;                  // map_variations.rs:23-26
			}
		};
		thread_ranges(m1 - m0, n_threads, [&](int, uint64_t a, uint64_t z) { work(m0 + a, m0 + z); });
		// ---- the device's ASCII buffer: anchors first, then every non-empty member sequence at a multiple of four ----
		std::vector<PrJob> jobs; std::vector<uint64_t> job_member; std::vector<PrSeg> segs;
		uint64_t cat = (h_anchor.size() + 3) & ~(uint64_t)3, words = 0;
		for (uint64_t m = m0; m < m1; ++m) {
			PrMember &M = pm[m - m0];
			// (a member without an aligned position, status 7, is built all the same: a letter the complement rejects comes first, status 9)
			if (M.len == 0 || M.status == 8 || M.status == 9) continue;          // status 9 from an edit letter: nothing reads the sequence
			jobs.push_back(PrJob{cat, (uint64_t)segs.size(), words, (uint32_t)M.segs.size(), M.len, promises[p0 + promise_of[m - m0]].reverse ? 1u : 0u, 0u});
			job_member.push_back(m);
			segs.insert(segs.end(), M.segs.begin(), M.segs.end());
			cat += ((uint64_t)M.len + 3) & ~(uint64_t)3; words += ((uint64_t)M.len + 3) / 4;
			std::vector<PrSeg>().swap(M.segs);
		}
		if (jobs.size() >= (1ULL << 31)) fail("more than 2^31 members in one chunk");
		DBuf<char> d_ascii(cat + 64);
		std::vector<uint32_t> rejected(jobs.size(), 0u);
		if (!h_anchor.empty()) PGA_HIP(hipMemcpyAsync(d_ascii.p, h_anchor.data(), h_anchor.size(), hipMemcpyHostToDevice, st));
		if (!jobs.empty()) {
			DBuf<char> d_cons(h_append.size() + 1), d_iseq(ih - il + 1);
			if (!h_append.empty()) PGA_HIP(hipMemcpyAsync(d_cons.p, h_append.data(), h_append.size(), hipMemcpyHostToDevice, st));
			if (ih > il) PGA_HIP(hipMemcpyAsync(d_iseq.p, ins_seq + il, ih - il, hipMemcpyHostToDevice, st));
			DBuf<PrJob> d_jobs; d_jobs.upload(jobs, st);
			DBuf<PrSeg> d_segs; d_segs.upload(segs, st);
			DBuf<uint32_t> d_rej(jobs.size()); d_rej.zero(st);
			const unsigned grid = (unsigned)std::min<uint64_t>((words + PR_THREADS - 1) / PR_THREADS, 8192);
			hipLaunchKernelGGL(k_promise_build, dim3(grid), dim3(PR_THREADS), 0, st, d_jobs.p, (int)jobs.size(), words, d_segs.p, d_cons.p, d_iseq.p, d_ascii.p, d_rej.p);
			PGA_HIP(hipGetLastError());
			rejected = d_rej.download(st);                                        // (synchronises: the host buffers above may go)
		} else PGA_HIP(sync_stream(st));
		for (size_t j = 0; j < jobs.size(); ++j) if (rejected[j]) { PrMember &M = pm[job_member[j] - m0]; M.status = 9; M.ms = M.bw = 0; }
		// ---- the stage tap ends here: status, band and the sequences as the aligner would read them ----
		if (stage) {
			std::vector<char> all = d_ascii.download(st);
			size_t j = 0;
			for (uint64_t m = m0; m < m1; ++m) {
				const PrMember &M = pm[m - m0];
				stage->status[m] = M.status; stage->mean_shift[m] = (int32_t)M.ms; stage->band_width[m] = (uint32_t)M.bw;
				while (j < jobs.size() && job_member[j] < m) ++j;
				if (M.status == 0 && M.len && j < jobs.size() && job_member[j] == m) stage->seqs.insert(stage->seqs.end(), all.begin() + jobs[j].dst, all.begin() + jobs[j].dst + M.len);
				stage->seq_off[m + 1] = stage->seqs.size();
			}
			p0 = p1;
			continue;
		}
		// ---- alignment of the members that got this far ----
		std::vector<MvDevJob> mvj; std::vector<uint64_t> mvj_member;
		for (size_t j = 0; j < jobs.size(); ++j) {
			const uint64_t m = job_member[j]; const PrMember &M = pm[m - m0];
			if (M.status != 0) continue;
			const int64_t p = p0 + promise_of[m - m0];
			if (M.ms < INT32_MIN || M.ms > INT32_MAX || M.bw > (int64_t)UINT32_MAX) fail("band parameters outside 32 bits (member " + std::to_string(m) + ")");
			mvj.push_back(MvDevJob{anchor_at[p - p0], jobs[j].dst, promises[p].anchor_len, M.len, (int32_t)M.ms, (uint32_t)M.bw});
			mvj_member.push_back(m);
		}
		std::vector<pga_mapvar_res_t> v_res(mvj.size());
		std::vector<pga_sub_t> v_subs; std::vector<pga_del_t> v_dels; std::vector<pga_ins_t> v_inss; std::vector<char> v_iseq;
		if (!mvj.empty()) { memset(v_res.data(), 0, v_res.size() * sizeof(pga_mapvar_res_t)); map_variations_dev((int64_t)mvj.size(), mvj.data(), d_ascii.p, cat, prm, v_res.data(), v_subs, v_dels, v_inss, v_iseq, st); }
		PGA_HIP(sync_stream(st));
		// ---- pack, member by member in input order ----
		size_t k = 0;
		for (uint64_t m = m0; m < m1; ++m) {
			const PrMember &M = pm[m - m0];
			pga_mapvar_res_t &o = res[m];
			memset(&o, 0, sizeof(o));
			o.sub_off = o_subs.size(); o.del_off = o_dels.size(); o.ins_off = o_inss.size();
			o.status = M.status;
			if (M.status != 0) continue;
			if (M.len == 0) { o.n_dels = 1; o_dels.push_back(pga_del_t{0u, promises[p0 + promise_of[m - m0]].anchor_len}); continue; }   // Edit::deleted (edits.rs:241-247)
			if (k >= mvj.size() || mvj_member[k] != m) fail("internal: a member lost its alignment job");
			const pga_mapvar_res_t &v = v_res[k++];
			o.status = v.status; o.score = v.score; o.attempts = v.attempts; o.hit_boundary = v.hit_boundary;
			o.n_subs = v.n_subs; o.n_dels = v.n_dels; o.n_inss = v.n_inss; o.n_ins_bases = v.n_ins_bases;
			o_subs.insert(o_subs.end(), v_subs.begin() + v.sub_off, v_subs.begin() + v.sub_off + v.n_subs);
			o_dels.insert(o_dels.end(), v_dels.begin() + v.del_off, v_dels.begin() + v.del_off + v.n_dels);
			for (uint32_t t = 0; t < v.n_inss; ++t) { const pga_ins_t &x = v_inss[v.ins_off + t]; o_inss.push_back(pga_ins_t{x.pos, x.len, (uint64_t)o_iseq.size()}); o_iseq.insert(o_iseq.end(), v_iseq.begin() + x.seq_off, v_iseq.begin() + x.seq_off + x.len); }
		}
		p0 = p1;
	}
}

} // namespace pga
