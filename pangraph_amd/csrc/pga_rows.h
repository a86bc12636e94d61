// pga_rows.h -- ROWS of letters built from consensus sequences and edit lists: the paths of pga_reconstruct.hip (reconstruct_run.rs:56-127) and
// the rows of the two exports of a finished graph (pga_export.hip: export block-sequences, pangraph_block.rs:135-189, and export core-genome,
// export_core_genome.rs:53-141).  A row is a list of (member, reverse) PIECES -- of a path: its nodes; a piece is Edit::apply_aligned (aligned
// mode, edits.rs:331-347) or Edit::apply (unaligned mode, edits.rs:307-329) of the member's edits to its block's consensus,
// reverse-complemented (io/seq.rs:9-33) when `reverse` is set.
//   host     the ROW TABLE, O(pieces + edits): per piece prepare_edit (pga_edits.h) and aligned_segments or promise_segments (pga_runs.h), the
//            piece's runs placed at the piece's offset in the row; the runs of a reverse piece are listed in reverse order and flagged ROW_REV,
//            so that the table of a row is ordered by built letter whatever the strands are.
//            Plain functions over the C-ABI arrays: a program without a device can call them (tests/emu/export_rows_emu.cpp).
//   device   k_rows, one thread per 16 letters: rows start at multiples of 16 in one UNIT space (a unit = 16 letters), a launch covers
//            the units [u0, u1) and stores unit u at out + 16 * (u - u0), always as one aligned 16-byte vector.  k_rows<true> also rotates
//            a row (Vec::rotate_right, reconstruct_run.rs:97) and compares it with the letters a caller expects.
// One job record serves both users: an export uploads eight bytes per row (rot, cmp) that its kernel never reads.
// Compiles under hipcc and, with dev/emu/hip_emu.h included first, under g++ -std=c++17 -DPGA_EMU.
#pragma once
#include "pga_runs.h"
#include <stdexcept>
#include <string>
#include <unordered_map>

namespace pga {

constexpr uint32_t ROW_REV = 4;                              // RowRun.kind: PrSeg's kind (0 consensus, 1 insertion, 2 one letter, 3 gap = PR_GAP) | ROW_REV
constexpr uint32_t ROW_BAD_COMP = 1, ROW_GAP = 2;            // per-row flags: a rejected complement, an emitted '-' (unaligned mode only)
constexpr int ROW_THREADS = 256, ROW_LETTERS = 16;           // a workgroup writes 4096 letters

// one run of a row: built letters [out, out of the next run) of the UNROTATED row.  Forward: letter out + k is source letter k (of
// cons[src ..] or ins_seq[src - ins_base ..], the one letter `src`, or '-'); reverse: the complement of source letter (run length - 1 - k).
struct RowRun { uint32_t out, kind; uint64_t src; };
// a row with at least one letter: unit0 is the first of its units among all units of the table; k_rows<true> only: rot is what the row is
// rotated right by (<= len), cmp whether it is compared with the expected letters
struct RowJob { uint64_t run_off, unit0; uint32_t n_run, len, rot, cmp; };
struct alignas(16) RowVec { uint32_t w[4]; };

static inline uint64_t row_pad(uint64_t len) { return (len + (ROW_LETTERS - 1)) & ~(uint64_t)(ROW_LETTERS - 1); }

__device__ __forceinline__ bool row_has_gap(uint32_t w)     // one of the four bytes is '-'
{
	const uint32_t x = w ^ 0x2d2d2d2du;
	return ((x - 0x01010101u) & ~x & 0x80808080u) != 0u;
}

// One thread per unit u of [u0, u1): the 16 WRITTEN letters i0 .. i0+15 of the row that holds the unit (the last unit of a row may be short;
// the bytes behind the row's last letter are written as 0).  A unit inside one consensus or insertion run takes one 16-byte load (reverse: the
// mirrored 16 bytes, complemented), a unit inside one gap run no load at all; every other unit goes letter by letter from run to run.
// gap_flag: ROW_GAP in unaligned mode (an emitted '-' is flagged), 0 in aligned mode.  out == nullptr: nothing is stored, only the flags.
// kRotCmp: written letter i is built letter (i + len - rot) mod len, the letter-by-letter walk goes on behind the seam of the rotation with
// the first run, and a job with `cmp` is compared with expected + 16 * (u - u0): its first difference (atomicMin) and their count.
// Without kRotCmp: rot, cmp, expected, first and count are not read.
template <bool kRotCmp>
__global__ __launch_bounds__(ROW_THREADS) void k_rows(const RowJob *__restrict__ jobs, int n_jobs, uint64_t u0, uint64_t u1, const RowRun *__restrict__ runs,
                                                      const char *__restrict__ cons, const char *__restrict__ ins_seq, uint64_t ins_base,
                                                      char *__restrict__ out, uint32_t *__restrict__ flags, uint32_t gap_flag,
                                                      const char *__restrict__ expected, unsigned long long *__restrict__ first, unsigned long long *__restrict__ count)
{
	__shared__ uint8_t s_comp[256];
	s_comp[threadIdx.x] = d_comp.t[threadIdx.x];
	__syncthreads();
	for (uint64_t u = u0 + (uint64_t)blockIdx.x * ROW_THREADS + threadIdx.x; u < u1; u += (uint64_t)gridDim.x * ROW_THREADS) {
		int lo = 0, hi = n_jobs - 1;                                        // the last job with unit0 <= u (jobs have at least one unit)
		while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].unit0 <= u) lo = mid; else hi = mid - 1; }
		const RowJob J = jobs[lo];
		const uint32_t i0 = (uint32_t)(u - J.unit0) * ROW_LETTERS;
		const uint32_t n = J.len - i0 < (uint32_t)ROW_LETTERS ? J.len - i0 : (uint32_t)ROW_LETTERS;
		const RowRun *R = runs + J.run_off;
		uint32_t b = i0;                                                    // built index of written letter i0
		if constexpr (kRotCmp) b = i0 >= J.rot ? i0 - J.rot : i0 + (J.len - J.rot);
		uint32_t a = 0, z = J.n_run - 1;                                    // the last run with out <= b
		while (a < z) { const uint32_t mid = (a + z + 1) >> 1; if (R[mid].out <= b) a = mid; else z = mid - 1; }
		RowRun g = R[a];
		uint32_t s_beg = g.out, s_end = a + 1 < J.n_run ? R[a + 1].out : J.len;
		uint32_t w[4] = {0u, 0u, 0u, 0u}, fl = 0u;
		const uint32_t kd0 = g.kind & 3u;
		if (n == (uint32_t)ROW_LETTERS && b + ROW_LETTERS <= s_end && kd0 == PR_GAP) {       // (inside one run: not across the seam either)
			w[0] = w[1] = w[2] = w[3] = 0x2d2d2d2du;                          // (the complement of '-' is '-')
			fl |= gap_flag;
		} else if (n == (uint32_t)ROW_LETTERS && b + ROW_LETTERS <= s_end && kd0 != 2u) {
			const char *base = kd0 == 0u ? cons + g.src : ins_seq + (g.src - ins_base);
			const uint32_t k0 = b - s_beg;
			if (!(g.kind & ROW_REV)) __builtin_memcpy(w, base + k0, 16);
			else {
				uint32_t v[4];
				__builtin_memcpy(v, base + ((s_end - s_beg) - ROW_LETTERS - k0), 16);
#pragma unroll
				for (int k = 0; k < ROW_LETTERS; ++k) {                           // written letter k: the complement of source byte 15 - k
					const uint32_t c = (v[(15 - k) >> 2] >> (8 * ((15 - k) & 3))) & 255u, cc = s_comp[c];
					if (!cc) fl |= ROW_BAD_COMP;
					w[k >> 2] |= (cc ? cc : c) << (8 * (k & 3));
				}
			}
			if (gap_flag && (row_has_gap(w[0]) || row_has_gap(w[1]) || row_has_gap(w[2]) || row_has_gap(w[3]))) fl |= gap_flag;
		} else {
#pragma unroll
			for (int k = 0; k < ROW_LETTERS; ++k) {
				if ((uint32_t)k < n) {
					if (b >= s_end || (kRotCmp && b < s_beg)) {                     // left the run: the next one (no run is empty), or behind the seam the first
						if (kRotCmp && b < s_beg) a = 0u; else ++a;
						g = R[a];
						s_beg = g.out; s_end = a + 1 < J.n_run ? R[a + 1].out : J.len;
					}
					const bool rev = (g.kind & ROW_REV) != 0u;
					const uint32_t kd = g.kind & 3u, off = rev ? s_end - 1u - b : b - s_beg;
					uint32_t c = kd == 0u ? (uint8_t)cons[g.src + off] : kd == 1u ? (uint8_t)ins_seq[g.src - ins_base + off] : kd == 2u ? (uint32_t)(g.src & 255u) : (uint32_t)'-';
					if (rev) { const uint32_t cc = s_comp[c]; if (cc) c = cc; else fl |= ROW_BAD_COMP; }
					if (c == (uint32_t)'-') fl |= gap_flag;
					w[k >> 2] |= c << (8 * (k & 3));
					++b;
					if (kRotCmp && b == J.len) b = 0u;
				}
			}
		}
		if (out) { RowVec v; v.w[0] = w[0]; v.w[1] = w[1]; v.w[2] = w[2]; v.w[3] = w[3]; *reinterpret_cast<RowVec*>(out + ROW_LETTERS * (u - u0)) = v; }
		if (fl) atomicOr(&flags[lo], fl);
		if constexpr (kRotCmp) {
			if (expected && J.cmp) {
				const RowVec e = *reinterpret_cast<const RowVec*>(expected + ROW_LETTERS * (u - u0));
				uint32_t d[4] = {w[0] ^ e.w[0], w[1] ^ e.w[1], w[2] ^ e.w[2], w[3] ^ e.w[3]};
				if (n < (uint32_t)ROW_LETTERS) {                                  // behind the row's last letter the expected buffer holds nothing
#pragma unroll
					for (int q = 0; q < 4; ++q) { const uint32_t have = n > 4u * q ? n - 4u * q : 0u; d[q] &= have >= 4u ? 0xffffffffu : (1u << (8u * have)) - 1u; }
				}
				if (d[0] | d[1] | d[2] | d[3]) {
					uint32_t cnt = 0u, fst = 0u;
#pragma unroll
					for (int k = ROW_LETTERS - 1; k >= 0; --k) if ((d[k >> 2] >> (8 * (k & 3))) & 255u) { ++cnt; fst = (uint32_t)k; }
					atomicMin(&first[lo], (unsigned long long)(i0 + fst));
					atomicAdd(&count[lo], (unsigned long long)cnt);
				}
			}
		}
	}
}

// ---------------------------------------------------------------- host side: the graph, validated, and the row table
// blocks, members and edits in the layout of pga_reconstruct (members numbered globally in block order)
struct RowGraph {
	int64_t n_blocks = 0; const pga_rc_block_t *blocks = nullptr; const pga_rc_member_t *members = nullptr;
	const pga_sub_t *subs = nullptr; const pga_del_t *dels = nullptr; const pga_ins_t *inss = nullptr; const char *ins_seq = nullptr;
	bool aligned = true;
	uint64_t n_mem = 0;
	std::vector<uint64_t> mem_first, sub_off, del_off, ins_off;
	std::vector<uint32_t> blk_of, mem_len;                              // per member: its block, its built length (aligned: cons_len; unaligned: prepare_edit's)
};
struct RowPiece { uint64_t member; uint32_t reverse, pad; };

// offsets and validation; throws std::runtime_error(who + ": " + what).  The members are checked in n_threads ranges (thread_ranges, pga_runs.h):
// pga_reconstruct takes range_threads(), the exports 1 -- on an MI355X host eight worker threads made an export call of 100 000 aligned
// members 3-4 ms slower, although the loop alone is faster with them.
static void row_graph_init(RowGraph &G, const std::string &who, int64_t n_blocks, const pga_rc_block_t *blocks, const pga_rc_member_t *members, const pga_sub_t *subs,
                           const pga_del_t *dels, const pga_ins_t *inss, const char *ins_seq, bool aligned, int n_threads)
{
	auto fail = [&](const std::string &what) { throw std::runtime_error(who + ": " + what); };
	if (n_blocks < 0 || (n_blocks && !blocks)) fail("null argument");
	if (n_blocks >= (1LL << 32)) fail("more than 2^32 blocks");
	G.n_blocks = n_blocks; G.blocks = blocks; G.members = members; G.subs = subs; G.dels = dels; G.inss = inss; G.ins_seq = ins_seq; G.aligned = aligned;
	G.mem_first.assign((size_t)n_blocks + 1, 0);
	for (int64_t b = 0; b < n_blocks; ++b) {
		if (blocks[b].cons_len && !blocks[b].consensus) fail("null consensus with a non-zero length (block " + std::to_string(b) + ")");
		if (blocks[b].cons_len >= (1u << 30)) fail("consensus longer than 2^30");
		G.mem_first[b + 1] = G.mem_first[b] + blocks[b].n_members;
	}
	const uint64_t n_mem = G.n_mem = G.mem_first[n_blocks];
	if (n_mem && !members) fail("null member list");
	G.blk_of.resize(n_mem);
	for (int64_t b = 0; b < n_blocks; ++b) for (uint64_t m = G.mem_first[b]; m < G.mem_first[b + 1]; ++m) G.blk_of[m] = (uint32_t)b;
	G.sub_off.assign(n_mem + 1, 0); G.del_off.assign(n_mem + 1, 0); G.ins_off.assign(n_mem + 1, 0);
	for (uint64_t m = 0; m < n_mem; ++m) { G.sub_off[m + 1] = G.sub_off[m] + members[m].n_subs; G.del_off[m + 1] = G.del_off[m] + members[m].n_dels; G.ins_off[m + 1] = G.ins_off[m] + members[m].n_inss; }
	if ((G.sub_off[n_mem] && !subs) || (G.del_off[n_mem] && !dels) || (G.ins_off[n_mem] && !inss)) fail("null edit list");
	G.mem_len.resize(n_mem);
	thread_ranges(n_mem, n_threads, [&](int, uint64_t m0, uint64_t m1) {
		PreparedEdit P;
		for (uint64_t m = m0; m < m1; ++m) {
			const uint32_t L = blocks[G.blk_of[m]].cons_len;
			uint64_t ins_letters = 0;
			for (uint64_t t = G.sub_off[m]; t < G.sub_off[m + 1]; ++t) {
				if (subs[t].pos >= L) fail("substitution beyond the consensus (member " + std::to_string(m) + ")");
				if (subs[t].alt > 255u) fail("substitution letter outside one byte (member " + std::to_string(m) + ")");
			}
			for (uint64_t t = G.del_off[m]; t < G.del_off[m + 1]; ++t) if ((uint64_t)dels[t].pos + dels[t].len > L) fail("deletion beyond the consensus (member " + std::to_string(m) + ")");
			for (uint64_t t = G.ins_off[m]; t < G.ins_off[m + 1]; ++t) {
				if (inss[t].pos > L) fail("insertion beyond the consensus (member " + std::to_string(m) + ")");
				if (!aligned && inss[t].len && !ins_seq) fail("null insertion letters with a non-zero length (member " + std::to_string(m) + ")");
				ins_letters += inss[t].len;
			}
			if (aligned) { G.mem_len[m] = L; continue; }                      // (apply_aligned: insertions are missing, every deleted position is a '-')
			if ((uint64_t)L + ins_letters > (1ULL << 31)) fail("member longer than 2^31 letters (member " + std::to_string(m) + ")");
			G.mem_len[m] = prepare_edit(subs + G.sub_off[m], members[m].n_subs, dels + G.del_off[m], members[m].n_dels, inss + G.ins_off[m], members[m].n_inss, ins_seq, L, P);
		}
	});
}

// the runs of one piece whose first letter is built letter `at` of its row and whose block's consensus lies at cons_base, appended to
// runs_out (RowRun.src of an insertion run is the offset in the caller's ins_seq); returns the piece's length.  P and segs are scratch.
static uint32_t row_piece_runs(const RowGraph &G, const RowPiece &piece, uint32_t at, uint64_t cons_base, std::vector<RowRun> &runs_out, PreparedEdit &P, std::vector<PrSeg> &segs)
{
	const uint64_t m = piece.member;
	const uint32_t L = G.blocks[G.blk_of[m]].cons_len, n_inss = G.aligned ? 0u : G.members[m].n_inss;
	const uint32_t applied = prepare_edit(G.subs + G.sub_off[m], G.members[m].n_subs, G.dels + G.del_off[m], G.members[m].n_dels, G.inss + G.ins_off[m], n_inss, G.ins_seq, L, P);
	segs.clear();
	const uint32_t built = G.aligned ? aligned_segments(P, L, cons_base, segs) : promise_segments(P, L, cons_base, 0, segs);
	if (built != (G.aligned ? L : applied) || built != G.mem_len[m]) throw std::runtime_error("internal: a piece's runs do not add up to its length");
	const uint32_t ns = (uint32_t)segs.size();
	if (!piece.reverse) for (uint32_t s = 0; s < ns; ++s) runs_out.push_back(RowRun{at + segs[s].out, segs[s].kind, segs[s].src});
	else for (uint32_t s = ns; s-- > 0;) runs_out.push_back(RowRun{at + (built - (s + 1 < ns ? segs[s + 1].out : built)), segs[s].kind | ROW_REV, segs[s].src});
	return built;
}

// the row table of some rows, in the order they were appended, and what the device needs beside it: one copy of every consensus a piece reads
// (RowRun.src of a consensus run points into `cons`) and the range [ins_lo, ins_hi) of the insertion letters the pieces point into (the kernel
// subtracts ins_base = ins_lo)
struct RowTable {
	std::vector<RowRun> runs; std::vector<RowJob> jobs; std::vector<uint64_t> job_row;
	std::vector<char> cons; std::unordered_map<uint32_t, uint64_t> cons_at; std::vector<uint32_t> cons_blocks;
	uint64_t ins_lo = UINT64_MAX, ins_hi = 0, units = 0;
	struct Mark { size_t runs, jobs, cons, cons_blocks; uint64_t ins_lo, ins_hi, units; };
	Mark mark() const { return Mark{runs.size(), jobs.size(), cons.size(), cons_blocks.size(), ins_lo, ins_hi, units}; }
	void undo(const Mark &k)                                              // takes the rows appended since mark() out again
	{
		runs.resize(k.runs); jobs.resize(k.jobs); job_row.resize(k.jobs); cons.resize(k.cons);
		while (cons_blocks.size() > k.cons_blocks) { cons_at.erase(cons_blocks.back()); cons_blocks.pop_back(); }
		ins_lo = k.ins_lo; ins_hi = k.ins_hi; units = k.units;
	}
	void clear() { runs.clear(); jobs.clear(); job_row.clear(); cons.clear(); cons_at.clear(); cons_blocks.clear(); ins_lo = UINT64_MAX; ins_hi = 0; units = 0; }
};

// what member m reads, in the table: its block's consensus (copied at its first use; returns where it lies) and its insertion letters
static uint64_t row_place(const RowGraph &G, uint64_t m, RowTable &T)
{
	const uint32_t b = G.blk_of[m];
	auto ins = T.cons_at.emplace(b, (uint64_t)T.cons.size());
	if (ins.second) { T.cons.insert(T.cons.end(), G.blocks[b].consensus, G.blocks[b].consensus + G.blocks[b].cons_len); T.cons_blocks.push_back(b); }
	if (!G.aligned) for (uint64_t t = G.ins_off[m]; t < G.ins_off[m + 1]; ++t) if (G.inss[t].len) { T.ins_lo = std::min<uint64_t>(T.ins_lo, G.inss[t].seq_off); T.ins_hi = std::max<uint64_t>(T.ins_hi, G.inss[t].seq_off + G.inss[t].len); }
	return ins.first->second;
}

// appends row `row` = pieces[0 .. n_pieces) to the table (an empty row adds nothing); returns its length.  P and segs are scratch.
static uint64_t row_append_row(const RowGraph &G, uint64_t row, const RowPiece *pieces, uint64_t n_pieces, RowTable &T, PreparedEdit &P, std::vector<PrSeg> &segs)
{
	const size_t run0 = T.runs.size();
	uint64_t at = 0;
	for (uint64_t q = 0; q < n_pieces; ++q) {
		const uint64_t m = pieces[q].member;
		if (m >= G.n_mem) throw std::runtime_error("internal: a piece names a member that does not exist");
		if (at + G.mem_len[m] > (1ULL << 31)) throw std::runtime_error("row over 2^31 letters (row " + std::to_string(row) + ")");
		if (!G.mem_len[m]) continue;                                        // (a piece without letters has no run)
		at += row_piece_runs(G, pieces[q], (uint32_t)at, row_place(G, m, T), T.runs, P, segs);
	}
	if (at) {
		T.jobs.push_back(RowJob{(uint64_t)run0, T.units, (uint32_t)(T.runs.size() - run0), (uint32_t)at, 0u, 0u});
		T.job_row.push_back(row);
		T.units += row_pad(at) / ROW_LETTERS;
	}
	return at;
}

} // namespace pga
