// pga_rows.h without a device: the row table built by the host builder (aligned and unaligned mode, forward and reverse pieces) and
// k_rows<false> run under dev/emu/hip_emu.h, tile by tile, into buffers allocated at exactly the size the kernel may touch -- under the address
// sanitizer a store or a 16-byte load one byte out is an error -- against a direct scalar construction of every row (Edit::apply_aligned,
// edits.rs:331-347, or Edit::apply without the stripping of '-', edits.rs:307-329; then the reverse complement, io/seq.rs:9-33).
// k_rows<true>, as pga_reconstruct.hip launches it, over unaligned rows that are rotated and compared with expected letters: against the
// same construction after rotate_right, and a scalar comparison with expected letters that differ where they were made to.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/export_rows_emu.cpp -o export_rows_emu && ./export_rows_emu
#include <cstdio>
#include <memory>
#include <random>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_rows.h"

using namespace pga;

struct Member { std::vector<pga_sub_t> subs; std::vector<pga_del_t> dels; std::vector<std::pair<uint32_t, std::string>> inss; };
struct Block { std::string cons; std::vector<Member> mem; };
struct Row { std::vector<RowPiece> pieces; };

// the C-ABI arrays of a graph
struct Flat {
	std::vector<pga_rc_block_t> B; std::vector<pga_rc_member_t> M; std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I; std::string letters;
	std::vector<uint64_t> first;
	explicit Flat(const std::vector<Block> &blocks)
	{
		letters.assign(7, '?');                                             // (the slice the chunk points into does not start at 0)
		first.push_back(0);
		for (const Block &b : blocks) {
			B.push_back(pga_rc_block_t{b.cons.data(), (uint32_t)b.cons.size(), (uint32_t)b.mem.size()});
			first.push_back(first.back() + b.mem.size());
			for (const Member &m : b.mem) {
				M.push_back(pga_rc_member_t{(uint32_t)m.subs.size(), (uint32_t)m.dels.size(), (uint32_t)m.inss.size()});
				S.insert(S.end(), m.subs.begin(), m.subs.end()); D.insert(D.end(), m.dels.begin(), m.dels.end());
				for (auto &x : m.inss) { I.push_back(pga_ins_t{x.first, (uint32_t)x.second.size(), (uint64_t)letters.size()}); letters += x.second; }
			}
		}
	}
};

// one piece, directly; flags as the kernel is to raise them
static std::string direct_piece(const Block &b, const Member &m, bool reverse, bool aligned, uint32_t &fl)
{
	const uint32_t L = (uint32_t)b.cons.size();
	std::vector<int> q(b.cons.begin(), b.cons.end());
	for (int &c : q) c &= 255;
	for (const pga_sub_t &s : m.subs) q[s.pos] = (int)s.alt;
	for (const pga_del_t &d : m.dels) for (uint32_t p = d.pos; p < d.pos + d.len; ++p) q[p] = aligned ? (int)'-' : -1;
	std::string s;
	if (aligned) for (int c : q) s.push_back((char)c);
	else {
		auto inss = m.inss;
		std::sort(inss.begin(), inss.end());                                // Ins: Ord by (pos, seq)
		size_t ii = 0;
		for (uint32_t p = 0; p <= L; ++p) {
			for (; ii < inss.size() && inss[ii].first == p; ++ii) s += inss[ii].second;
			if (p < L && q[p] >= 0) s.push_back((char)q[p]);
		}
		if (s.find('-') != std::string::npos) fl |= ROW_GAP;
	}
	if (!reverse) return s;
	std::string r(s.size(), '?');
	for (size_t i = 0; i < s.size(); ++i) {
		const uint8_t c = (uint8_t)s[s.size() - 1 - i], cc = h_comp.t[c];
		if (!cc) fl |= ROW_BAD_COMP;
		r[i] = (char)(cc ? cc : c);                                          // (a rejected letter is emitted unchanged)
	}
	return r;
}

template <class T> static std::unique_ptr<T[]> exact(const T *src, size_t n)      // a heap block of exactly n elements (n == 0: one the kernel must not touch)
{
	std::unique_ptr<T[]> p(new T[n ? n : 1]);
	if (n) memcpy(p.get(), src, n * sizeof(T));
	return p;
}

static long n_rows_checked = 0, n_tiles_run = 0, n_rev = 0, n_bad = 0, n_gap_rows = 0, n_empty_between = 0, n_vec_gap_units = 0;

// builds the table of `rows` (all in one chunk), runs the kernel over tiles of tile_units and compares; false on a difference
static bool check(const std::vector<Block> &blocks, const std::vector<Row> &rows, bool aligned, uint64_t tile_units, const char *what)
{
	Flat F(blocks);
	RowGraph G;
	row_graph_init(G, "emu", (int64_t)F.B.size(), F.B.data(), F.M.data(), F.S.data(), F.D.data(), F.I.data(), F.letters.data(), aligned, 1);
	RowTable T; PreparedEdit P; std::vector<PrSeg> segs;
	std::vector<std::string> want(rows.size()); std::vector<uint32_t> want_fl(rows.size(), 0u);
	for (size_t r = 0; r < rows.size(); ++r) {
		size_t nonempty_seen = 0; bool empty_pending = false;
		for (const RowPiece &pc : rows[r].pieces) {
			const uint32_t b = G.blk_of[pc.member];
			const std::string s = direct_piece(blocks[b], blocks[b].mem[pc.member - F.first[b]], pc.reverse != 0, aligned, want_fl[r]);
			if (s.empty() && nonempty_seen) empty_pending = true;
			if (!s.empty()) { if (empty_pending) { ++n_empty_between; empty_pending = false; } ++nonempty_seen; }
			want[r] += s;
			n_rev += pc.reverse != 0;
		}
		if (r == rows.size() / 2) {                                           // a row appended and taken out again leaves the table as it was
			const RowTable::Mark mk = T.mark();
			row_append_row(G, r, rows[r].pieces.data(), rows[r].pieces.size(), T, P, segs);
			T.undo(mk);
			if (T.runs.size() != mk.runs || T.jobs.size() != mk.jobs || T.job_row.size() != mk.jobs || T.cons.size() != mk.cons || T.cons_at.size() != T.cons_blocks.size() || T.units != mk.units) { fprintf(stderr, "%s: undo does not restore the table\n", what); return false; }
		}
		const uint64_t len = row_append_row(G, r, rows[r].pieces.data(), rows[r].pieces.size(), T, P, segs);
		if (len != want[r].size()) { fprintf(stderr, "%s: row %zu: the builder says %llu letters, the direct construction %zu\n", what, r, (unsigned long long)len, want[r].size()); return false; }
	}
	for (size_t j = 0; j < T.jobs.size(); ++j) {
		const RowJob &J = T.jobs[j];
		for (uint32_t s = 0; s < J.n_run; ++s) {
			const RowRun &R = T.runs[J.run_off + s];
			const uint32_t end = s + 1 < J.n_run ? T.runs[J.run_off + s + 1].out : J.len;
			if (end <= R.out || (s == 0 && R.out != 0)) { fprintf(stderr, "%s: row %llu: run table not ordered, not from 0 or with an empty run\n", what, (unsigned long long)T.job_row[j]); return false; }
			if ((R.kind & 3u) == PR_GAP) for (uint32_t u = (R.out + 15u) / 16u; (u + 1) * 16u <= end; ++u) ++n_vec_gap_units;
		}
	}
	const size_t n_jobs = T.jobs.size();
	if (!n_jobs) { n_rows_checked += (long)rows.size(); return true; }
	const uint64_t ins_lo = T.ins_lo < T.ins_hi ? T.ins_lo : 0, ins_n = T.ins_lo < T.ins_hi ? T.ins_hi - T.ins_lo : 0;
	auto d_jobs = exact(T.jobs.data(), n_jobs); auto d_runs = exact(T.runs.data(), T.runs.size());
	auto d_cons = exact(T.cons.data(), T.cons.size()); auto d_iseq = exact(F.letters.data() + ins_lo, ins_n);
	const uint32_t gap_flag = aligned ? 0u : ROW_GAP;
	std::vector<std::string> got(rows.size());
	std::vector<uint32_t> fl(n_jobs, 0u), fl_null(n_jobs, 0u);
	auto d_fl = exact(fl.data(), n_jobs); auto d_fl_null = exact(fl_null.data(), n_jobs);
	size_t jc = 0;
	for (uint64_t a = 0; a < T.units; a += tile_units) {
		const uint64_t z = std::min(T.units, a + tile_units);
		std::unique_ptr<char[]> tile(new char[(z - a) * ROW_LETTERS]);
		memset(tile.get(), '#', (z - a) * ROW_LETTERS);
		const unsigned grid = (unsigned)((z - a + ROW_THREADS - 1) / ROW_THREADS);
		emu_launch(dim3(grid), dim3(ROW_THREADS), [&] { k_rows<false>(d_jobs.get(), (int)n_jobs, a, z, d_runs.get(), d_cons.get(), d_iseq.get(), ins_lo, tile.get(), d_fl.get(), gap_flag, nullptr, nullptr, nullptr); });
		++n_tiles_run;
		while (jc < n_jobs) {                                                 // the tile's segments, as the host driver cuts them
			const RowJob &J = T.jobs[jc];
			if (J.unit0 >= z) break;
			const uint64_t from = std::max(J.unit0, a), row_off = (from - J.unit0) * ROW_LETTERS, row_end = std::min<uint64_t>(J.len, (z - J.unit0) * ROW_LETTERS);
			if (got[T.job_row[jc]].size() != row_off) { fprintf(stderr, "%s: segments out of order\n", what); return false; }
			got[T.job_row[jc]].append(tile.get() + (from - a) * ROW_LETTERS, row_end - row_off);
			if (J.unit0 + row_pad(J.len) / ROW_LETTERS > z) break;
			++jc;
		}
	}
	// out == nullptr: one grid-stride launch over everything (fewer workgroups than tiles of 256 units), only the flags
	emu_launch(dim3((unsigned)std::max<uint64_t>(1, T.units / 700)), dim3(ROW_THREADS), [&] { k_rows<false>(d_jobs.get(), (int)n_jobs, (uint64_t)0, T.units, d_runs.get(), d_cons.get(), d_iseq.get(), ins_lo, (char*)nullptr, d_fl_null.get(), gap_flag, nullptr, nullptr, nullptr); });
	std::vector<uint32_t> row_fl(rows.size(), 0u), row_fl_null(rows.size(), 0u);
	for (size_t j = 0; j < n_jobs; ++j) { row_fl[T.job_row[j]] = d_fl[j]; row_fl_null[T.job_row[j]] = d_fl_null[j]; }
	for (size_t r = 0; r < rows.size(); ++r) {
		if (got[r] != want[r]) {
			size_t i = 0; while (i < got[r].size() && i < want[r].size() && got[r][i] == want[r][i]) ++i;
			fprintf(stderr, "%s (%s, tiles of %llu units): row %zu of %zu letters differs at letter %zu\n", what, aligned ? "aligned" : "unaligned", (unsigned long long)tile_units, r, want[r].size(), i);
			return false;
		}
		if (row_fl[r] != want_fl[r] || row_fl_null[r] != want_fl[r]) { fprintf(stderr, "%s (%s): row %zu: flags %u, without output %u, expected %u\n", what, aligned ? "aligned" : "unaligned", r, row_fl[r], row_fl_null[r], want_fl[r]); return false; }
		n_bad += (want_fl[r] & ROW_BAD_COMP) != 0; n_gap_rows += (want_fl[r] & ROW_GAP) != 0;
	}
	n_rows_checked += (long)rows.size();
	return true;
}

// ---------------------------------------------------------------- k_rows<true>: rotated and compared rows
// mode 0: compared with the letters it is to have; 1: compared with letters that differ at the first and the last letter, on both sides of
// the seam of the rotation and of a 16-letter edge; 2: not compared (its stretch of the expected buffer holds nothing to compare with)
struct RotRow { std::vector<RowPiece> pieces; uint64_t rot_val; int mode; };       // rotated right by rot_val % (len + 1)
static long n_rot_rows = 0, n_rotated = 0, n_seam_later = 0, n_one_at_seam = 0, n_cmp_rows = 0, n_planted_rows = 0, n_planted = 0, n_uncompared = 0, n_short_tail_cmp = 0;

static bool check_rot(const std::vector<Block> &blocks, const std::vector<RotRow> &rows, const char *what)
{
	Flat F(blocks);
	RowGraph G;
	row_graph_init(G, "emu", (int64_t)F.B.size(), F.B.data(), F.M.data(), F.S.data(), F.D.data(), F.I.data(), F.letters.data(), false, range_threads());
	RowTable T; PreparedEdit P; std::vector<PrSeg> segs;
	std::vector<std::string> want(rows.size()), expd(rows.size()); std::vector<uint32_t> want_fl(rows.size(), 0u);
	std::vector<unsigned long long> want_first(rows.size(), ~0ULL), want_count(rows.size(), 0ULL);
	for (size_t r = 0; r < rows.size(); ++r) {
		std::string s; size_t first_piece = 0;
		for (const RowPiece &pc : rows[r].pieces) {
			const uint32_t b = G.blk_of[pc.member];
			s += direct_piece(blocks[b], blocks[b].mem[pc.member - F.first[b]], pc.reverse != 0, false, want_fl[r]);
			if (!first_piece) first_piece = s.size();
		}
		const uint64_t len = row_append_row(G, r, rows[r].pieces.data(), rows[r].pieces.size(), T, P, segs);
		if (len != s.size()) { fprintf(stderr, "%s: row %zu: the builder says %llu letters, the direct construction %zu\n", what, r, (unsigned long long)len, s.size()); return false; }
		if (!len) continue;
		RowJob &J = T.jobs.back();
		const uint32_t rot = (uint32_t)(rows[r].rot_val % (len + 1));
		J.rot = rot; J.cmp = rows[r].mode != 2;
		if (rot && rot < len) {
			++n_rotated;
			n_seam_later += len - rot >= first_piece;                         // written letter 0 is a letter of a later piece
			n_one_at_seam += (T.runs[J.run_off].kind & 3u) == 2u && (T.runs[J.run_off + J.n_run - 1].kind & 3u) == 2u;
		}
		std::rotate(s.rbegin(), s.rbegin() + rot, s.rend());                  // Vec::rotate_right
		want[r] = expd[r] = s;
		if (rows[r].mode == 1) {
			const int64_t at[] = {0, (int64_t)len - 1, (int64_t)rot - 1, (int64_t)rot, 15, 16};
			for (int64_t i : at) if (i >= 0 && i < (int64_t)len && expd[r][i] == want[r][i]) { expd[r][i] = want[r][i] == 'A' ? 'C' : 'A'; ++n_planted; }
			++n_planted_rows;
		}
		if (rows[r].mode == 2) { expd[r].assign(len, '!'); ++n_uncompared; }
		else {
			++n_cmp_rows; n_short_tail_cmp += len % 16 != 0;
			for (size_t i = len; i-- > 0;) if (expd[r][i] != want[r][i]) { ++want_count[r]; want_first[r] = i; }
		}
	}
	n_rot_rows += (long)rows.size();
	const size_t n_jobs = T.jobs.size();
	if (!n_jobs) return true;
	const uint64_t ins_lo = T.ins_lo < T.ins_hi ? T.ins_lo : 0, ins_n = T.ins_lo < T.ins_hi ? T.ins_hi - T.ins_lo : 0;
	auto d_jobs = exact(T.jobs.data(), n_jobs); auto d_runs = exact(T.runs.data(), T.runs.size());
	auto d_cons = exact(T.cons.data(), T.cons.size()); auto d_iseq = exact(F.letters.data() + ins_lo, ins_n);
	// out and expected of exactly the padded size; behind a row's last letter the expected buffer holds what no row has
	const size_t bytes = (size_t)T.units * ROW_LETTERS;
	std::unique_ptr<char[]> d_out(new char[bytes]), d_exp(new char[bytes]);
	memset(d_out.get(), '#', bytes); memset(d_exp.get(), '#', bytes);
	for (size_t j = 0; j < n_jobs; ++j) memcpy(d_exp.get() + T.jobs[j].unit0 * ROW_LETTERS, expd[T.job_row[j]].data(), T.jobs[j].len);
	const std::vector<uint32_t> zero(n_jobs, 0u); const std::vector<unsigned long long> none(n_jobs, ~0ULL), nought(n_jobs, 0ULL);
	for (int pass = 0; pass < 2; ++pass) {                                  // with an output buffer, then without (a grid-stride launch of fewer workgroups)
		auto d_fl = exact(zero.data(), n_jobs); auto d_first = exact(none.data(), n_jobs); auto d_count = exact(nought.data(), n_jobs);
		const unsigned grid = pass == 0 ? (unsigned)((T.units + ROW_THREADS - 1) / ROW_THREADS) : (unsigned)std::max<uint64_t>(1, T.units / 700);
		emu_launch(dim3(grid), dim3(ROW_THREADS), [&] { k_rows<true>(d_jobs.get(), (int)n_jobs, (uint64_t)0, T.units, d_runs.get(), d_cons.get(), d_iseq.get(), ins_lo, pass == 0 ? d_out.get() : (char*)nullptr, d_fl.get(), ROW_GAP, d_exp.get(), d_first.get(), d_count.get()); });
		for (size_t j = 0; j < n_jobs; ++j) {
			const size_t r = (size_t)T.job_row[j]; const RowJob &J = T.jobs[j];
			if (pass == 0) {
				const char *got = d_out.get() + J.unit0 * ROW_LETTERS;
				for (uint64_t i = 0; i < row_pad(J.len); ++i) if (got[i] != (i < J.len ? want[r][i] : '\0')) {
					fprintf(stderr, "%s: rotated row %zu of %u letters, rotated by %u, differs at letter %llu\n", what, r, J.len, J.rot, (unsigned long long)i);
					return false;
				}
			}
			if (d_fl[j] != want_fl[r]) { fprintf(stderr, "%s: rotated row %zu (pass %d): flags %u, expected %u\n", what, r, pass, d_fl[j], want_fl[r]); return false; }
			if (d_first[j] != want_first[r] || d_count[j] != want_count[r]) {
				fprintf(stderr, "%s: rotated row %zu of %u letters, rotated by %u, mode %d (pass %d): first difference %lld, count %llu, expected %lld, %llu\n", what, r, J.len, J.rot, rows[r].mode, pass,
				        (long long)d_first[j], d_count[j], (long long)want_first[r], want_count[r]);
				return false;
			}
		}
	}
	return true;
}

int main()
{
	std::mt19937_64 rng(20261018);
	auto below = [&](uint64_t n) { return (uint32_t)(rng() % n); };
	const char alphabet[] = "ACGTYRWSKMDVHBN-";
	auto letter = [&](int it) -> char { return below(400) == 0 ? "xXa"[below(3)] : alphabet[below(it % 3 ? 4 : (below(8) ? 15 : 16))]; };
	const uint32_t edge_lens[] = {0, 1, 15, 16, 17, 4095, 4096, 4097};

	// ---- 1. directed: every edge length as a row of its own, forward and reverse, plain, with a substitution at the first and at the last letter,
	//         and between two other pieces; gap runs that start or end at unit offsets 15, 16, 17 and cover whole units; whole-consensus deletions
	{
		std::vector<Block> blocks; std::vector<Row> rows;
		uint64_t m = 0;
		auto add = [&](const std::string &cons, Member mem) { blocks.push_back(Block{cons, {mem}}); return m++; };
		auto random_cons = [&](uint32_t L) { std::string s(L, 'A'); for (char &c : s) c = alphabet[below(15)]; return s; };
		const uint64_t five = add(random_cons(5), Member{});
		for (uint32_t L : edge_lens) {
			const uint64_t plain = add(random_cons(L), Member{});
			Member ends; if (L) { ends.subs.push_back(pga_sub_t{0u, (uint32_t)'T'}); ends.subs.push_back(pga_sub_t{L - 1, (uint32_t)'G'}); ends.subs.push_back(pga_sub_t{L - 1, (uint32_t)'C'}); }
			const uint64_t with_ends = add(random_cons(L), ends);
			Member whole; if (L) { whole.dels.push_back(pga_del_t{0u, L}); whole.subs.push_back(pga_sub_t{L / 2, (uint32_t)'x'}); }
			const uint64_t gone = add(random_cons(L), whole);
			for (uint32_t rev = 0; rev < 2; ++rev) {
				rows.push_back(Row{{RowPiece{plain, rev, 0}}});
				rows.push_back(Row{{RowPiece{with_ends, rev, 0}}});
				rows.push_back(Row{{RowPiece{gone, rev, 0}}});
				rows.push_back(Row{{RowPiece{five, 1u - rev, 0}, RowPiece{plain, rev, 0}, RowPiece{five, rev, 0}}});
				rows.push_back(Row{{RowPiece{five, rev, 0}, RowPiece{gone, rev, 0}, RowPiece{with_ends, 1u - rev, 0}}});
			}
		}
		const uint32_t starts[] = {0, 15, 16, 17, 31, 32, 33}, ends[] = {15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 100};
		for (uint32_t s : starts) for (uint32_t e : ends) if (e > s) {
			Member g; g.dels.push_back(pga_del_t{s, e - s});
			g.subs.push_back(pga_sub_t{s, (uint32_t)'G'});                      // under the deletion
			if (e < 100) { g.subs.push_back(pga_sub_t{e, (uint32_t)'T'}); g.subs.push_back(pga_sub_t{e, (uint32_t)'R'}); }   // right behind it, twice
			const uint64_t id = add(random_cons(100), g);
			for (uint32_t rev = 0; rev < 2; ++rev) { rows.push_back(Row{{RowPiece{id, rev, 0}}}); rows.push_back(Row{{RowPiece{five, 0, 0}, RowPiece{id, rev, 0}, RowPiece{id, 1u - rev, 0}}}); }
		}
		for (int aligned = 0; aligned < 2; ++aligned)
			for (uint64_t tile : {(uint64_t)256, (uint64_t)1 << 40})
				if (!check(blocks, rows, aligned != 0, tile, "directed")) return 1;
	}

	// ---- 1b. k_rows<true>, directed: every edge length as a row of one piece (plain, and with one-letter runs at the first and the last letter:
	//          on both sides of the seam) and as a row of three pieces, forward and reverse, rotated by 0, 1, 15, 16, 17, len-1 and len; every row
	//          once with planted differences and once either compared clean or not compared
	{
		std::vector<Block> blocks; std::vector<RotRow> rows;
		uint64_t m = 0;
		auto add = [&](const std::string &cons, Member mem) { blocks.push_back(Block{cons, {mem}}); return m++; };
		auto random_cons = [&](uint32_t L) { std::string s(L, 'A'); for (char &c : s) c = alphabet[below(15)]; return s; };
		const uint64_t five = add(random_cons(5), Member{});
		int alt = 0;
		for (uint32_t L : edge_lens) if (L) {
			const uint64_t plain = add(random_cons(L), Member{});
			Member ends; ends.subs.push_back(pga_sub_t{0u, (uint32_t)'T'}); ends.subs.push_back(pga_sub_t{L - 1, (uint32_t)'G'});
			const uint64_t with_ends = add(random_cons(L), ends);
			const uint64_t mid = L >= 15 ? add(random_cons(L - 10), Member{}) : 0;
			std::vector<uint32_t> rots;
			for (uint32_t rot : {0u, 1u, 15u, 16u, 17u, L - 1, L}) if (rot <= L && std::find(rots.begin(), rots.end(), rot) == rots.end()) rots.push_back(rot);
			for (uint32_t rot : rots) for (uint32_t rev = 0; rev < 2; ++rev) {
				std::vector<std::vector<RowPiece>> shapes{{RowPiece{plain, rev, 0}}, {RowPiece{with_ends, rev, 0}}};
				if (L >= 15) shapes.push_back({RowPiece{five, 1u - rev, 0}, RowPiece{mid, rev, 0}, RowPiece{five, rev, 0}});
				for (auto &sh : shapes) { rows.push_back(RotRow{sh, rot, 1}); rows.push_back(RotRow{sh, rot, ++alt % 3 ? 0 : 2}); }
			}
		}
		if (!check_rot(blocks, rows, "directed, rotated")) return 1;
	}

	// ---- 2. random graphs ----
	const uint32_t lens[] = {0, 1, 2, 15, 16, 17, 31, 32, 33, 64, 100, 257, 257, 100, 64, 40};
	for (int it = 0; it < 40; ++it) {
		std::vector<Block> blocks; std::vector<Row> rows;
		std::vector<uint64_t> first{0};
		const uint32_t nb = 4 + below(12);
		for (uint32_t b = 0; b < nb; ++b) {
			Block blk;
			const uint32_t L = it % 10 == 0 && b == 0 ? 4090 + below(12) : lens[below(sizeof(lens) / sizeof(lens[0]))];
			blk.cons.resize(L); for (char &c : blk.cons) c = letter(it);
			const uint32_t nm = 1 + below(4);
			for (uint32_t j = 0; j < nm; ++j) {
				Member mem;
				const int shape = (int)below(8);
				if (L) {
					for (uint32_t k = below(5); k-- > 0;) {
						const uint32_t pos = below(L), len = below(L - pos + 1);
						mem.dels.push_back(pga_del_t{pos, shape == 1 ? std::min(len, 20u) : len});
						if (shape == 2 && pos + len < L) mem.dels.push_back(pga_del_t{pos + len, below(L - pos - len + 1)});     // adjacent
						if (shape == 3 && len) mem.dels.push_back(pga_del_t{pos + below(len), 1u});                              // inside another
					}
					if (shape == 4) mem.dels.push_back(pga_del_t{0u, L});
					if (shape == 5) { mem.dels.push_back(pga_del_t{0u, L / 2}); mem.dels.push_back(pga_del_t{L / 2, L - L / 2}); }
					if (shape >= 6) mem.dels.clear();
					for (uint32_t k = below(8); k-- > 0;) {
						const uint32_t pos = below(3) ? below(L) : (below(2) ? 0u : L - 1);
						mem.subs.push_back(pga_sub_t{pos, (uint32_t)(uint8_t)letter(it)});
						if (below(3) == 0) mem.subs.push_back(pga_sub_t{pos, (uint32_t)(uint8_t)letter(it)});
					}
					for (const pga_del_t &d : mem.dels) if (d.len && below(2)) mem.subs.push_back(pga_sub_t{d.pos + below(d.len), (uint32_t)'G'});   // under a deletion
					for (size_t i = mem.subs.size(); i > 1; --i) std::swap(mem.subs[i - 1], mem.subs[below(i)]);
				}
				for (uint32_t k = below(4); k-- > 0;) {
					std::string s(below(4) ? below(8) : 16 + below(40), 'A'); for (char &c : s) c = letter(it);
					const uint32_t pos = below(L + 1);
					mem.inss.emplace_back(pos, s);
					if (below(4) == 0) { std::string s2(1 + below(20), 'A'); for (char &c : s2) c = letter(it); mem.inss.emplace_back(pos, s2); }      // two at one position
				}
				blk.mem.push_back(mem);
			}
			first.push_back(first.back() + nm);
			blocks.push_back(blk);
		}
		const uint32_t nr = 20 + below(30);
		for (uint32_t r = 0; r < nr; ++r) {
			Row row;
			for (uint32_t k = below(7); k-- > 0;) row.pieces.push_back(RowPiece{below(first.back()), below(2), 0u});
			rows.push_back(row);
		}
		for (int aligned = 0; aligned < 2; ++aligned)
			if (!check(blocks, rows, aligned != 0, it % 3 == 0 ? 256 : it % 3 == 1 ? 512 : (uint64_t)1 << 40, "random")) return 1;
		std::vector<RotRow> rot_rows;
		for (const Row &row : rows) rot_rows.push_back(RotRow{row.pieces, below(4) ? rng() : (uint64_t)0, (int)below(3)});
		if (!check_rot(blocks, rot_rows, "random, rotated")) return 1;
	}
	if (n_rows_checked < 3000 || !n_rev || n_bad < 5 || n_gap_rows < 5 || !n_empty_between || n_vec_gap_units < 20 || n_tiles_run < 100) {
		fprintf(stderr, "the generator missed a shape: rows %ld, reverse pieces %ld, rejected complements %ld, rows with an emitted '-' %ld, empty pieces between others %ld, whole gap units %ld, tiles %ld\n",
		        n_rows_checked, n_rev, n_bad, n_gap_rows, n_empty_between, n_vec_gap_units, n_tiles_run);
		return 1;
	}
	if (n_rot_rows < 1500 || n_rotated < 800 || n_seam_later < 100 || n_one_at_seam < 40 || n_cmp_rows < 800 || n_planted_rows < 500 || n_planted < 2000 || n_uncompared < 200 || n_short_tail_cmp < 400) {
		fprintf(stderr, "the generator missed a rotated shape: rows %ld, rotated %ld, written from a later piece %ld, one-letter runs at the seam %ld, compared %ld, with planted differences %ld (%ld letters), not compared %ld, compared with a short last unit %ld\n",
		        n_rot_rows, n_rotated, n_seam_later, n_one_at_seam, n_cmp_rows, n_planted_rows, n_planted, n_uncompared, n_short_tail_cmp);
		return 1;
	}
	printf("export_rows_emu OK: %ld rows, %ld tiles, %ld reverse pieces, %ld rows with a rejected complement, %ld with an emitted '-', %ld empty pieces between others, %ld whole gap units; "
	       "%ld rotated of %ld rows for k_rows<true> (%ld written from a later piece, %ld with one-letter runs at the seam), %ld compared (%ld with a short last unit), "
	       "%ld with %ld planted differences, %ld not compared\n",
	       n_rows_checked, n_tiles_run, n_rev, n_bad, n_gap_rows, n_empty_between, n_vec_gap_units, n_rotated, n_rot_rows, n_seam_later, n_one_at_seam, n_cmp_rows, n_short_tail_cmp,
	       n_planted_rows, n_planted, n_uncompared);
	return 0;
}
