// pga_reconstruct.hip -- reconstruct (packages/pangraph/src/commands/reconstruct/reconstruct_run.rs:56-127) for all paths of a graph: blocks
// with their members' edit lists and the node chains of the paths in, every path's sequence out -- or, in verify mode, only whether it is
// the sequence the caller expects.
//   edits.rs:307-329          Edit::apply of a node's edits to its block's consensus
//   io/seq.rs:9-33            reverse_complement of a node on the reverse strand
//   reconstruct_run.rs:82-97  concatenation, the length check, rotate_right by the first node's position
// What runs where:
//   host     list bookkeeping, O(nodes + edits): validation (all of it before anything is launched), every member's built length, and one
//            RUN TABLE per path: per node prepare_edit and promise_segments (pga_edits.h, pga_runs.h), the node's runs placed at the node's
//            offset in the path; the runs of a reverse node are listed in reverse order and flagged "read backwards and complement", so
//            that the table of a path is ordered by built letter whatever the strands are.  Empty nodes contribute no run.
//   device   k_reconstruct, one thread per 16 written letters: the rotation and the mirrored index of reverse runs are on the load side,
//            the store is one aligned 16-byte vector; the comparison with the expected letters is fused (verify-only stores nothing)
// Paths are processed in chunks whose built letters stay under PGA_RECON_CHUNK_MB (default 2048; a longer single path is a chunk of its
// own).  Per chunk the device receives the runs, one copy of every consensus a node of the chunk reads, the slice of the insertion letters
// its members point into and, in verify mode, the expected letters.  The result does not depend on the chunking.
#include "pga_common.h"
#include "../../include/pga_align.h"
#include "pga_runs.h"
#include <exception>
#include <thread>
#include <unordered_map>

namespace pga {

constexpr uint32_t RC_REV = 4;                               // RcRun.kind: PrSeg's kind (0 consensus, 1 insertion, 2 one letter) | RC_REV
constexpr uint32_t RC_BAD_COMP = 1, RC_GAP = 2;              // per-path flags: a rejected complement, an emitted '-'
constexpr int RC_THREADS = 256, RC_LETTERS = 16;             // a workgroup writes a tile of 4096 letters
constexpr int RC_BUSY_FAMILY = 15;                           // pga_busy_end (include/pga_align.h)

// one run of a path: built letters [out, out of the next run) of the UNROTATED path.  Forward: letter out + k is source letter k (of
// cons[src ..] or ins_seq[src ..], or the one letter `src`); reverse: the complement of source letter (run length - 1 - k).
struct RcRun { uint32_t out, kind; uint64_t src; };
// dst: offset of the path in the output and in the expected buffer (a multiple of 16); unit0: the first of its 16-letter units among all
// units of the launch; rot: what the path is rotated right by (<= len); cmp: compare with the expected letters
struct RcJob { uint64_t dst, run_off, unit0; uint32_t n_run, len, rot, cmp; };

__device__ __forceinline__ bool rc_has_gap(uint32_t w)      // one of the four bytes is '-'
{
	const uint32_t x = w ^ 0x2d2d2d2du;
	return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u;
}

// One thread per 16 WRITTEN letters i0 .. i0+15 of a path.  Written letter i is built letter (i + len - rot) mod len (Vec::rotate_right).
// A thread whose 16 letters lie in one run of consensus or insertion letters copies them with one 16-byte load; every other thread goes
// letter by letter and moves on to the next run (after the seam of the rotation: to the first) when a letter leaves its run.
__global__ __launch_bounds__(RC_THREADS) void k_reconstruct(const RcJob *__restrict__ jobs, int n_jobs, uint64_t n_units, const RcRun *__restrict__ runs,
                                                            const char *__restrict__ cons, const char *__restrict__ ins_seq, char *__restrict__ out,
                                                            const char *__restrict__ expected, uint32_t *__restrict__ flags,
                                                            unsigned long long *__restrict__ first, unsigned long long *__restrict__ count)
{
	__shared__ uint8_t s_comp[256];
	s_comp[threadIdx.x] = d_comp.t[threadIdx.x];
	__syncthreads();
	for (uint64_t u = (uint64_t)blockIdx.x * RC_THREADS + threadIdx.x; u < n_units; u += (uint64_t)gridDim.x * RC_THREADS) {
		int lo = 0, hi = n_jobs - 1;                                        // the last job with unit0 <= u (jobs have at least one unit)
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].unit0 <= u) lo = mid; else hi = mid - 1; }
		const RcJob J = jobs[lo];
		const uint32_t i0 = (uint32_t)(u - J.unit0) * RC_LETTERS;
		const uint32_t n = min((uint32_t)RC_LETTERS, J.len - i0);           // letters of this unit (the last unit of a path may be short)
		const RcRun *R = runs + J.run_off;
		uint32_t b = i0 >= J.rot ? i0 - J.rot : i0 + (J.len - J.rot);       // built index of written letter i0
		uint32_t a = 0, z = J.n_run - 1;                                    // the last run with out <= b
		while (a < z) { const uint32_t mid = (a + z + 1) >> 1; if (R[mid].out <= b) a = mid; else z = mid - 1; }
		RcRun g = R[a];
		uint32_t s_beg = g.out, s_end = a + 1 < J.n_run ? R[a + 1].out : J.len;
		uint32_t w[4] = {0u, 0u, 0u, 0u}, fl = 0u;
		if (n == RC_LETTERS && b + RC_LETTERS <= s_end && (g.kind & 3u) != 2u) {      // (inside one run: not across the seam either)
			const char *base = (g.kind & 3u) == 0u ? cons : ins_seq;
			const uint32_t k0 = b - s_beg;
			if (!(g.kind & RC_REV)) __builtin_memcpy(w, base + g.src + k0, 16);
			else {
				uint32_t v[4];
				__builtin_memcpy(v, base + g.src + ((s_end - s_beg) - RC_LETTERS - k0), 16);
#pragma unroll
				for (int k = 0; k < RC_LETTERS; ++k) {                            // written letter k: the complement of source byte 15 - k
					const uint32_t c = (v[(15 - k) >> 2] >> (8 * ((15 - k) & 3))) & 255u, cc = s_comp[c];
					if (!cc) fl |= RC_BAD_COMP;
					w[k >> 2] |= (cc ? cc : c) << (8 * (k & 3));
				}
			}
			if (rc_has_gap(w[0]) || rc_has_gap(w[1]) || rc_has_gap(w[2]) || rc_has_gap(w[3])) fl |= RC_GAP;
		} else {
#pragma unroll
			for (int k = 0; k < RC_LETTERS; ++k) {
				if ((uint32_t)k < n) {
					if (b < s_beg || b >= s_end) {                                  // left the run: the next one (no run is empty), or behind the seam the first
						a = b < s_beg ? 0u : min(a + 1u, J.n_run - 1u);
						g = R[a];
						s_beg = g.out; s_end = a + 1 < J.n_run ? R[a + 1].out : J.len;
					}
					const bool rev = (g.kind & RC_REV) != 0u;
					const uint32_t kd = g.kind & 3u, off = rev ? s_end - 1u - b : b - s_beg;
					uint32_t c = kd == 0u ? (uint8_t)cons[g.src + off] : kd == 1u ? (uint8_t)ins_seq[g.src + off] : (uint32_t)(g.src & 255u);
					if (rev) { const uint32_t cc = s_comp[c]; if (cc) c = cc; else fl |= RC_BAD_COMP; }
					if (c == (uint32_t)'-') fl |= RC_GAP;
					w[k >> 2] |= c << (8 * (k & 3));
					if (++b == J.len) b = 0u;
				}
			}
		}
		if (out) *reinterpret_cast<uint4*>(out + J.dst + i0) = make_uint4(w[0], w[1], w[2], w[3]);
		if (fl) atomicOr(&flags[lo], fl);
		if (expected && J.cmp) {
			const uint4 e = *reinterpret_cast<const uint4*>(expected + J.dst + i0);
			uint32_t d[4] = {w[0] ^ e.x, w[1] ^ e.y, w[2] ^ e.z, w[3] ^ e.w};
			if (n < (uint32_t)RC_LETTERS) {                                     // behind the path's last letter the expected buffer holds nothing
#pragma unroll
				for (int q = 0; q < 4; ++q) { const uint32_t have = n > 4u * q ? n - 4u * q : 0u; d[q] &= have >= 4u ? 0xffffffffu : (1u << (8u * have)) - 1u; }
			}
			if (d[0] | d[1] | d[2] | d[3]) {
				uint32_t cnt = 0u, fst = 0u;
#pragma unroll
				for (int k = RC_LETTERS - 1; k >= 0; --k) if ((d[k >> 2] >> (8 * (k & 3))) & 255u) { ++cnt; fst = (uint32_t)k; }
				atomicMin(&first[lo], (unsigned long long)(i0 + fst));
				atomicAdd(&count[lo], (unsigned long long)cnt);
			}
		}
	}
}

// ---------------------------------------------------------------- host side
static size_t recon_chunk_bytes()
{
	const char *e = getenv("PGA_RECON_CHUNK_MB");
	const double mb = e ? atof(e) : 2048.0;
	return (size_t)(std::max(mb, 1.0) * (double)(1u << 20));
}

// f(a, z) over [0, n) in contiguous ranges on a few host threads (range t is the t-th in order); exceptions are passed on
template <class F> static void rc_ranges(uint64_t n, int n_threads, F f)
{
	if (n < 64 || n_threads <= 1) { f(0, (uint64_t)0, n); return; }
	const uint64_t per = (n + (uint64_t)n_threads - 1) / (uint64_t)n_threads;
	std::vector<std::thread> th; std::vector<std::exception_ptr> err((size_t)n_threads);
	for (int t = 0; t < n_threads; ++t) th.emplace_back([&, t]() { try { f(t, std::min(n, per * t), std::min(n, per * (t + 1))); } catch (...) { err[t] = std::current_exception(); } });
	for (auto &x : th) x.join();
	for (auto &e : err) if (e) std::rethrow_exception(e);
}

static inline uint64_t rc_pad(uint64_t len) { return (len + (RC_LETTERS - 1)) & ~(uint64_t)(RC_LETTERS - 1); }

void reconstruct_host(int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs, const pga_del_t *dels, const pga_ins_t *inss,
                      const char *ins_seq, int64_t n_paths, const pga_recon_path_t *paths, const pga_recon_node_t *nodes, const char *const *expected,
                      const uint64_t *expected_len, pga_recon_res_t *res, char **out_seq)
{
	auto fail = [](const std::string &what) { throw std::runtime_error("pga_reconstruct: " + what); };
	const bool verify = expected != nullptr, write = out_seq != nullptr;
	// ---- offsets and validation: everything that fails the call does so here, before anything is launched ----
	if (n_blocks >= (1LL << 32)) fail("more than 2^32 blocks");
	std::vector<uint64_t> mem_first((size_t)n_blocks + 1, 0);
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (blocks[b].cons_len && !blocks[b].consensus) fail("null consensus with a non-zero length (block " + std::to_string(b) + ")");
		if (blocks[b].cons_len >= (1u << 30)) fail("consensus longer than 2^30");
		mem_first[b + 1] = mem_first[b] + blocks[b].n_members;
	}
	const uint64_t n_mem = mem_first[n_blocks];
	if (n_mem && !members) fail("null member list");
	std::vector<uint32_t> blk_of(n_mem);
	for (int64_t b = 0; b < n_blocks; ++b) for (uint64_t m = mem_first[b]; m < mem_first[b + 1]; ++m) blk_of[m] = (uint32_t)b;
	std::vector<uint64_t> sub_off(n_mem + 1, 0), del_off(n_mem + 1, 0), ins_off(n_mem + 1, 0);
	for (uint64_t m = 0; m < n_mem; ++m) { sub_off[m + 1] = sub_off[m] + members[m].n_subs; del_off[m + 1] = del_off[m] + members[m].n_dels; ins_off[m + 1] = ins_off[m] + members[m].n_inss; }
	if ((sub_off[n_mem] && !subs) || (del_off[n_mem] && !dels) || (ins_off[n_mem] && !inss)) fail("null edit list");
	const int n_threads = (int)std::min<unsigned>(8, std::max(1u, std::thread::hardware_concurrency()));
	std::vector<uint32_t> mem_len(n_mem);                                 // the built length of every member
	rc_ranges(n_mem, n_threads, [&](int, uint64_t a, uint64_t z) {
		PreparedEdit P;
		for (uint64_t m = a; m < z; ++m) {
			const uint32_t L = blocks[blk_of[m]].cons_len;
			uint64_t ins_letters = 0;
			for (uint64_t t = sub_off[m]; t < sub_off[m + 1]; ++t) {
				if (subs[t].pos >= L) fail("substitution beyond the consensus (member " + std::to_string(m) + ")");
				if (subs[t].alt > 255u) fail("substitution letter outside one byte (member " + std::to_string(m) + ")");
			}
			for (uint64_t t = del_off[m]; t < del_off[m + 1]; ++t) if ((uint64_t)dels[t].pos + dels[t].len > L) fail("deletion beyond the consensus (member " + std::to_string(m) + ")");
			for (uint64_t t = ins_off[m]; t < ins_off[m + 1]; ++t) {
				if (inss[t].pos > L) fail("insertion beyond the consensus (member " + std::to_string(m) + ")");
				if (inss[t].len && !ins_seq) fail("null insertion letters with a non-zero length (member " + std::to_string(m) + ")");
				ins_letters += inss[t].len;
			}
			if ((uint64_t)L + ins_letters > (1ULL << 31)) fail("member longer than 2^31 letters (member " + std::to_string(m) + ")");
			mem_len[m] = prepare_edit(subs + sub_off[m], members[m].n_subs, dels + del_off[m], members[m].n_dels, inss + ins_off[m], members[m].n_inss, ins_seq, L, P);
		}
	});
	if (n_paths && (!paths || !res)) fail("null path list");
	if (verify && !expected_len) fail("expected sequences without their lengths");
	std::vector<uint64_t> node_first((size_t)n_paths + 1, 0);
	for (int64_t p = 0; p < n_paths; ++p) node_first[p + 1] = node_first[p] + paths[p].n_nodes;
	if (node_first[n_paths] && !nodes) fail("null node list");
	// per path: the built length, the status as far as the host knows it, the place in the output (every path at a multiple of 16)
	std::vector<uint64_t> len((size_t)n_paths), dst((size_t)n_paths + 1, 0);
	std::vector<int32_t> status((size_t)n_paths, 0);
	for (int64_t p = 0; p < n_paths; ++p) {
		uint64_t l = 0;
		for (uint64_t k = node_first[p]; k < node_first[p + 1]; ++k) {
			if (nodes[k].member >= n_mem) fail("node names a member that does not exist (path " + std::to_string(p) + ", node " + std::to_string(k - node_first[p]) + ")");
			l += mem_len[nodes[k].member];
			if (l > (1ULL << 31)) fail("path longer than 2^31 letters (path " + std::to_string(p) + ")");
		}
		if (verify && expected_len[p] && !expected[p]) fail("null expected sequence with a non-zero length (path " + std::to_string(p) + ")");
		len[p] = l;
		if (paths[p].n_nodes) {                                               // (a path without nodes: Seq::new(), nothing is checked)
			if (l != paths[p].tot_len) status[p] = 1;
			else if (paths[p].first_pos > l) status[p] = 4;
		}
		if (status[p] == 0 && verify && expected_len[p] != l) status[p] = 5;
		dst[p + 1] = dst[p] + rc_pad(l);
	}
	struct Owned { char *p = nullptr; ~Owned() { free(p); } } obuf;
	if (write) { obuf.p = (char*)malloc((size_t)dst[n_paths] + 1); if (!obuf.p) fail("out of host memory"); }
	struct Stream { hipStream_t s; Stream() : s(stream_lease()) {} ~Stream() { stream_release(s); } } stream;
	hipStream_t st = stream.s;
	const size_t chunk_cap = recon_chunk_bytes();
	int64_t p0 = 0;
	while (p0 < n_paths) {
		// ---- the chunk: paths p0 .. p1 ----
		int64_t p1 = p0 + 1;
		while (p1 < n_paths && dst[p1 + 1] - dst[p0] <= chunk_cap) ++p1;
		const uint64_t k0 = node_first[p0], k1 = node_first[p1], chunk_letters = dst[p1] - dst[p0];
		std::vector<uint32_t> flags((size_t)(p1 - p0), 0u);
		std::vector<unsigned long long> first((size_t)(p1 - p0), ~0ULL), count((size_t)(p1 - p0), 0ULL);
		if (chunk_letters) {
			// one copy of every consensus a node reads, the slice of the insertion letters the members point into, every node's offset in its path
			std::unordered_map<uint32_t, uint64_t> cons_at;
			std::vector<char> h_cons;
			std::vector<uint32_t> node_out((size_t)(k1 - k0));
			uint64_t il = UINT64_MAX, ih = 0;
			for (int64_t p = p0; p < p1; ++p) {
				uint32_t o = 0;
				for (uint64_t k = node_first[p]; k < node_first[p + 1]; ++k) {
					const uint64_t m = nodes[k].member; const uint32_t b = blk_of[m];
					node_out[k - k0] = o; o += mem_len[m];
					if (cons_at.emplace(b, (uint64_t)h_cons.size()).second) h_cons.insert(h_cons.end(), blocks[b].consensus, blocks[b].consensus + blocks[b].cons_len);
					for (uint64_t t = ins_off[m]; t < ins_off[m + 1]; ++t) if (inss[t].len) { il = std::min<uint64_t>(il, inss[t].seq_off); ih = std::max<uint64_t>(ih, inss[t].seq_off + inss[t].len); }
				}
			}
			if (il > ih) il = ih = 0;
			// ---- the runs of every node, in node order (a few host threads, nodes are independent) ----
			std::vector<std::vector<RcRun>> part((size_t)n_threads);
			std::vector<uint32_t> node_runs((size_t)(k1 - k0), 0u);
			rc_ranges(k1 - k0, n_threads, [&](int t, uint64_t a, uint64_t z) {
				PreparedEdit P; std::vector<PrSeg> segs; std::vector<RcRun> &out = part[t];
				for (uint64_t k = k0 + a; k < k0 + z; ++k) {
					const uint64_t m = nodes[k].member; const uint32_t b = blk_of[m], L = blocks[b].cons_len;
					prepare_edit(subs + sub_off[m], members[m].n_subs, dels + del_off[m], members[m].n_dels, inss + ins_off[m], members[m].n_inss, ins_seq, L, P);
					segs.clear();
					const uint32_t built = promise_segments(P, L, cons_at.find(b)->second, il, segs);
					if (built != mem_len[m]) fail("internal: a member's runs do not add up to its length");
					const uint32_t at = node_out[k - k0], ns = (uint32_t)segs.size();
					if (!nodes[k].reverse) for (uint32_t s = 0; s < ns; ++s) out.push_back(RcRun{at + segs[s].out, segs[s].kind, segs[s].src});
					else for (uint32_t s = ns; s-- > 0;) out.push_back(RcRun{at + (built - (s + 1 < ns ? segs[s + 1].out : built)), segs[s].kind | RC_REV, segs[s].src});
					node_runs[k - k0] = ns;
				}
			});
			std::vector<RcRun> runs;
			for (auto &v : part) { runs.insert(runs.end(), v.begin(), v.end()); std::vector<RcRun>().swap(v); }
			std::vector<RcJob> jobs; std::vector<int64_t> job_path;
			uint64_t run_off = 0, units = 0;
			for (int64_t p = p0; p < p1; ++p) {
				uint64_t nr = 0;
				for (uint64_t k = node_first[p]; k < node_first[p + 1]; ++k) nr += node_runs[k - k0];
				if (len[p]) {
					jobs.push_back(RcJob{dst[p] - dst[p0], run_off, units, (uint32_t)nr, (uint32_t)len[p], status[p] == 1 || status[p] == 4 ? 0u : (uint32_t)paths[p].first_pos,
					                     verify && status[p] == 0 ? 1u : 0u});
					job_path.push_back(p);
					units += rc_pad(len[p]) / RC_LETTERS;
				}
				run_off += nr;
			}
			if (run_off != runs.size()) fail("internal: the run tables do not add up");
			if (jobs.size() >= (1ULL << 31)) fail("more than 2^31 paths in one chunk");
			// ---- the device ----
			DBuf<char> d_cons(h_cons.size() + 16), d_iseq(ih - il + 16), d_out, d_exp;
			if (!h_cons.empty()) PGA_HIP(hipMemcpyAsync(d_cons.p, h_cons.data(), h_cons.size(), hipMemcpyHostToDevice, st));
			if (ih > il) PGA_HIP(hipMemcpyAsync(d_iseq.p, ins_seq + il, ih - il, hipMemcpyHostToDevice, st));
			if (write) d_out.alloc(chunk_letters);
			if (verify) {
				d_exp.alloc(chunk_letters);
				for (const RcJob &J : jobs) if (J.cmp) PGA_HIP(hipMemcpyAsync(d_exp.p + J.dst, expected[job_path[&J - jobs.data()]], J.len, hipMemcpyHostToDevice, st));
			}
			DBuf<RcJob> d_jobs; d_jobs.upload(jobs, st);
			DBuf<RcRun> d_runs; d_runs.upload(runs, st);
			DBuf<uint32_t> d_flags(jobs.size()); d_flags.zero(st);
			DBuf<unsigned long long> d_first(jobs.size()), d_count(jobs.size());
			PGA_HIP(hipMemsetAsync(d_first.p, 0xff, jobs.size() * sizeof(unsigned long long), st));
			d_count.zero(st);
			const unsigned grid = (unsigned)std::min<uint64_t>((units + RC_THREADS - 1) / RC_THREADS, 2048);
			{
				EventTimer et(st);
				hipLaunchKernelGGL(k_reconstruct, dim3(grid), dim3(RC_THREADS), 0, st, d_jobs.p, (int)jobs.size(), units, d_runs.p, d_cons.p, d_iseq.p,
				                   write ? d_out.p : nullptr, verify ? d_exp.p : nullptr, d_flags.p, d_first.p, d_count.p);
				PGA_HIP(hipGetLastError());
				et.finish(RC_BUSY_FAMILY);                                          // (synchronises: the host buffers above may go)
			}
			Downloads dl(st);
			std::vector<uint32_t> j_flags; std::vector<unsigned long long> j_first, j_count;
			dl.add(j_flags, d_flags.p, jobs.size());
			if (verify) { dl.add(j_first, d_first.p, jobs.size()); dl.add(j_count, d_count.p, jobs.size()); }
			if (write) PGA_HIP(hipMemcpyAsync(obuf.p + dst[p0], d_out.p, chunk_letters, hipMemcpyDeviceToHost, st));
			dl.wait();
			PGA_HIP(sync_stream(st));
			for (size_t j = 0; j < jobs.size(); ++j) {
				const size_t q = (size_t)(job_path[j] - p0);
				flags[q] = j_flags[j];
				if (verify && jobs[j].cmp) { first[q] = j_first[j]; count[q] = j_count[j]; }
			}
		}
		// ---- the verdicts, in the order of include/pga_align.h: 2, 3, then what the host knew (1, 4, 5) ----
		for (int64_t p = p0; p < p1; ++p) {
			const size_t q = (size_t)(p - p0);
			pga_recon_res_t &o = res[p];
			memset(&o, 0, sizeof(o));
			o.status = (flags[q] & RC_BAD_COMP) ? 2 : (flags[q] & RC_GAP) ? 3 : status[p];
			o.len = len[p];
			o.seq_off = write && o.status == 0 ? dst[p] : 0;
			o.first_mismatch = -1; o.n_mismatch = 0;
			if (verify && o.status == 0 && count[q]) { o.first_mismatch = (int64_t)first[q]; o.n_mismatch = (int64_t)count[q]; }
		}
		p0 = p1;
	}
	if (write) { *out_seq = obuf.p; obuf.p = nullptr; }
}

} // namespace pga
