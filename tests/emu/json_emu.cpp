// pga_json_idx.h without a device: validation and the host tables, then every kernel of the header (and the graph checks of pga_topo_idx.h,
// the scan kernels of pga_gfa_idx.h) under dev/emu/hip_emu.h, with every buffer allocated at exactly the size the kernels may touch (under the
// address sanitizer an access one entry out is an error), against a direct scalar construction of serde_json's pretty writer over the
// reference's three BTreeMaps: std::map by id, a formatter that knows only "begin, entry, end" and nothing of the emitter's literals.
// The graphs are the named cases of tests/json_gen.py, dumped by tests/test_json_cpu.py as flat binary (one file per case, given as
// arguments) together with the text and the tables of the Python restatement: the emulated kernels, the direct construction and the
// restatement must agree in every byte.  The tiles are cut at several sizes and the insertion chunk is varied; std::stable_sort stands
// in for the two radix sorts.  Without arguments only the built-in checks run.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/json_emu.cpp -o json_emu && ./json_emu case.bin ...
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <numeric>
#include <string>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_json_idx.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
};
static std::string g_case = "built-in";
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "json_emu: %s:%d: %s (case %s)\n", __FILE__, __LINE__, #c, g_case.c_str()); return false; } } while (0)

struct Case {
	std::vector<pga_topo_block_t> B; std::vector<pga_topo_path_t> P; std::vector<pga_topo_node_t> N;
	std::vector<std::string> cons; std::vector<bool> cons_null;
	std::vector<pga_rc_member_t> M; std::vector<pga_sub_t> S; std::vector<pga_del_t> D; std::vector<pga_ins_t> I; std::string letters;
	std::vector<uint64_t> tot; std::vector<std::string> names, descs; std::vector<bool> name_null, desc_null;
	std::string want; std::vector<uint64_t> want_sec, want_path, want_block; std::vector<uint32_t> want_order; bool has_want = false;
	// the pointers of the call
	std::vector<const char*> cons_p, names_p, descs_p; std::vector<uint32_t> name_len, desc_len;
	void point()
	{
		cons_p.clear(); names_p.clear(); descs_p.clear(); name_len.clear(); desc_len.clear();
		for (size_t b = 0; b < cons.size(); ++b) cons_p.push_back(cons_null[b] ? nullptr : cons[b].data());
		for (size_t p = 0; p < names.size(); ++p) {
			names_p.push_back(name_null[p] ? nullptr : names[p].data()); name_len.push_back((uint32_t)names[p].size());
			descs_p.push_back(desc_null[p] ? nullptr : descs[p].data()); desc_len.push_back((uint32_t)descs[p].size());
		}
	}
};
struct Out { std::string text; std::vector<uint64_t> sec, path_off, block_off; std::vector<uint32_t> order; };

// emu_launch of dev/emu/hip_emu.h with the fibers and their stacks kept between launches: the header allocates 64 MB for every launch,
// and the cases here take thousands of them
// barriers == false: a kernel without __syncthreads() needs no fibers, its threads run one after the other (a barrier met there is a crash)
template <class F> static void launch(dim3 grid, dim3 block, F kernel_call, bool barriers = false)
{
	static std::vector<emu::Fiber> fb;
	gridDim = grid; blockDim = block;
	if (!barriers) {
		emu::cur = nullptr;
		for (unsigned b = 0; b < grid.x; ++b) for (unsigned t = 0; t < block.x; ++t) { blockIdx = dim3(b); threadIdx = dim3(t); kernel_call(); }
		return;
	}
	std::function<void()> fn = kernel_call;
	emu::body = &fn;
	if (fb.size() < block.x) { fb = std::vector<emu::Fiber>(block.x); for (emu::Fiber &f : fb) f.stack.resize(256 * 1024); }
	for (unsigned b = 0; b < grid.x; ++b) {
		blockIdx = dim3(b);
		for (unsigned t = 0; t < block.x; ++t) {
			emu::Fiber &f = fb[t];
			getcontext(&f.ctx);
			f.ctx.uc_stack.ss_sp = f.stack.data(); f.ctx.uc_stack.ss_size = f.stack.size(); f.ctx.uc_link = nullptr;
			makecontext(&f.ctx, (void (*)())emu::entry, 0);
			f.done = false;
		}
		for (unsigned alive = block.x; alive;) {
			unsigned waiting = 0, left = 0;
			for (unsigned t = 0; t < block.x; ++t) {
				emu::Fiber &f = fb[t];
				if (f.done) continue;
				threadIdx = dim3(t); emu::cur = &f; f.at_barrier = false;
				swapcontext(&emu::main_ctx, &f.ctx);
				if (f.done) ++left; else ++waiting;
			}
			if (waiting && left) { fprintf(stderr, "json_emu: workgroup %u: %u threads left the kernel while %u wait at a barrier\n", b, left, waiting); abort(); }
			alive = waiting;
		}
	}
	emu::body = nullptr; emu::cur = nullptr;
}

// ---------------------------------------------------------------- the dump of tests/test_json_cpu.py
struct Reader {
	std::string buf; size_t at = 0; bool ok = true;
	template <class T> T get() { T v{}; if (at + sizeof(T) > buf.size()) { ok = false; return v; } memcpy(&v, buf.data() + at, sizeof(T)); at += sizeof(T); return v; }
	template <class T> void vec(std::vector<T> &v, uint64_t n) { v.resize(n); if (at + n * sizeof(T) > buf.size()) { ok = false; return; } if (n) memcpy((void*)v.data(), buf.data() + at, n * sizeof(T)); at += n * sizeof(T); }
	std::string str(uint64_t n) { if (at + n > buf.size()) { ok = false; return ""; } std::string s = buf.substr(at, n); at += n; return s; }
	std::string opt(bool &null) { const uint32_t n = get<uint32_t>(); null = n == JS_NULL; return null ? std::string() : str(n); }
};
static bool load(const char *file, Case &G)
{
	FILE *f = fopen(file, "rb");
	if (!f) return false;
	Reader R; char tmp[1 << 16]; size_t n;
	while ((n = fread(tmp, 1, sizeof(tmp), f)) > 0) R.buf.append(tmp, n);
	fclose(f);
	if (R.str(8) != "PGAJSON1") return false;
	uint64_t c[9];
	for (uint64_t &x : c) x = R.get<uint64_t>();
	R.vec(G.B, c[0]); R.vec(G.P, c[1]); R.vec(G.N, c[2]);
	for (uint64_t b = 0; b < c[0]; ++b) { bool null; G.cons.push_back(R.opt(null)); G.cons_null.push_back(null); }
	R.vec(G.M, c[3]); R.vec(G.S, c[4]); R.vec(G.D, c[5]); R.vec(G.I, c[6]); G.letters = R.str(c[7]);
	for (uint64_t p = 0; p < c[1]; ++p) {
		bool a, b;
		G.tot.push_back(R.get<uint64_t>()); G.names.push_back(R.opt(a)); G.name_null.push_back(a); G.descs.push_back(R.opt(b)); G.desc_null.push_back(b);
	}
	G.want = R.str(c[8]); G.has_want = true;
	R.vec(G.want_sec, 3); R.vec(G.want_path, c[1]); R.vec(G.want_block, c[0]); R.vec(G.want_order, c[2]);
	G.point();
	return R.ok && R.at == R.buf.size();
}

// ---------------------------------------------------------------- the direct construction: serde_json's PrettyFormatter over BTreeMaps
struct Pretty {
	std::string s; std::vector<bool> has;
	void begin(char c) { s += c; has.push_back(false); }
	void entry() { s += has.back() ? ",\n" : "\n"; s.append(2 * has.size(), ' '); has.back() = true; }
	void end(char c) { const bool any = has.back(); has.pop_back(); if (any) { s += '\n'; s.append(2 * has.size(), ' '); } s += c; }
	void key(const std::string &k) { entry(); s += '"' + k + "\": "; }
	void num(uint64_t v) { s += std::to_string(v); }
	void str(const std::string &v)
	{
		s += '"';
		for (unsigned char c : v) {
			char u[8];
			if (c == '"') s += "\\\""; else if (c == '\\') s += "\\\\"; else if (c == 8) s += "\\b"; else if (c == 12) s += "\\f"; else if (c == 10) s += "\\n";
			else if (c == 13) s += "\\r"; else if (c == 9) s += "\\t"; else if (c < 32) { snprintf(u, sizeof(u), "\\u%04x", c); s += u; } else s += (char)c;
		}
		s += '"';
	}
	void opt(const std::string &v, bool null) { if (null) s += "null"; else str(v); }
};
static Out direct(const Case &G)
{
	Out D;
	Pretty W;
	std::vector<uint64_t> slot_first(G.B.size() + 1, 0), so(G.M.size() + 1, 0), d_o(G.M.size() + 1, 0), io(G.M.size() + 1, 0);
	for (size_t b = 0; b < G.B.size(); ++b) slot_first[b + 1] = slot_first[b] + (G.B[b].alive ? G.B[b].depth : 0);
	for (size_t m = 0; m < G.M.size(); ++m) { so[m + 1] = so[m] + G.M[m].n_subs; d_o[m + 1] = d_o[m] + G.M[m].n_dels; io[m + 1] = io[m] + G.M[m].n_inss; }
	std::map<uint64_t, uint32_t> node_at;
	std::map<uint64_t, std::map<uint64_t, uint64_t>> align;                 // block id -> node id -> slot
	std::vector<uint64_t> path_of(G.N.size());
	for (size_t p = 0; p < G.P.size(); ++p) for (uint64_t i = G.P[p].node_off; i < G.P[p].node_off + G.P[p].n_nodes; ++i) path_of[i] = G.P[p].path_id;
	for (uint32_t i = 0; i < G.N.size(); ++i) { node_at[G.N[i].node_id] = i; align[G.B[G.N[i].block].block_id][G.N[i].node_id] = slot_first[G.N[i].block] + G.N[i].member; }
	D.block_off.assign(G.B.size(), ~0ULL);
	W.begin('{');
	W.key("paths"); D.sec.push_back(W.s.size() - 9); W.begin('{');
	for (size_t p = 0; p < G.P.size(); ++p) {                              // (ascending path_id is input order: validated)
		const std::string id = std::to_string(G.P[p].path_id);
		W.key(id); D.path_off.push_back(W.s.size() - id.size() - 4); W.begin('{');
		W.key("id"); W.num(G.P[p].path_id);
		W.key("nodes"); W.begin('[');
		for (uint64_t i = G.P[p].node_off; i < G.P[p].node_off + G.P[p].n_nodes; ++i) { W.entry(); W.num(G.N[i].node_id); }
		W.end(']');
		W.key("tot_len"); W.num(G.tot[p]); W.key("circular"); W.s += G.P[p].circular ? "true" : "false";
		W.key("name"); W.opt(G.names[p], G.name_null[p]); W.key("desc"); W.opt(G.descs[p], G.desc_null[p]);
		W.end('}');
	}
	W.end('}');
	W.key("blocks"); D.sec.push_back(W.s.size() - 10); W.begin('{');
	for (size_t b = 0; b < G.B.size(); ++b) {                              // (the alive blocks ascend in id: validated)
		if (!G.B[b].alive) continue;
		const std::string id = std::to_string(G.B[b].block_id);
		W.key(id); D.block_off[b] = W.s.size() - id.size() - 4; W.begin('{');
		W.key("id"); W.num(G.B[b].block_id); W.key("consensus"); W.s += '"' + G.cons[b] + '"';
		W.key("alignments"); W.begin('{');
		for (auto &kv : align[G.B[b].block_id]) {
			const uint64_t m = kv.second;
			W.key(std::to_string(kv.first)); W.begin('{');
			W.key("subs"); W.begin('[');
			for (uint64_t k = so[m]; k < so[m + 1]; ++k) { W.entry(); W.begin('{'); W.key("pos"); W.num(G.S[k].pos); W.key("alt"); W.str(std::string(1, (char)G.S[k].alt)); W.end('}'); }
			W.end(']');
			W.key("dels"); W.begin('[');
			for (uint64_t k = d_o[m]; k < d_o[m + 1]; ++k) { W.entry(); W.begin('{'); W.key("pos"); W.num(G.D[k].pos); W.key("len"); W.num(G.D[k].len); W.end('}'); }
			W.end(']');
			W.key("inss"); W.begin('[');
			for (uint64_t k = io[m]; k < io[m + 1]; ++k) { W.entry(); W.begin('{'); W.key("pos"); W.num(G.I[k].pos); W.key("seq"); W.str(G.letters.substr(G.I[k].seq_off, G.I[k].len)); W.end('}'); }
			W.end(']');
			W.end('}');
		}
		W.end('}');
		W.end('}');
	}
	W.end('}');
	W.key("nodes"); D.sec.push_back(W.s.size() - 9); W.begin('{');
	for (auto &kv : node_at) {
		const pga_topo_node_t &N = G.N[kv.second];
		D.order.push_back(kv.second);
		W.key(std::to_string(kv.first)); W.begin('{');
		W.key("id"); W.num(N.node_id); W.key("block_id"); W.num(G.B[N.block].block_id); W.key("path_id"); W.num(path_of[kv.second]);
		W.key("strand"); W.s += N.reverse ? "\"-\"" : "\"+\"";
		W.key("position"); W.begin('['); W.entry(); W.num(N.pos0); W.entry(); W.num(N.pos1); W.end(']');
		W.end('}');
	}
	W.end('}');
	W.end('}');
	D.text = W.s;
	return D;
}

// ---------------------------------------------------------------- the kernels in the order of pga_json.hip
struct ScanBufs {
	Exact<gf_u64> tile_sum, tile_off, off; GfScan S; TsArray<gf_u64> val;
	ScanBufs(const gf_u64 *val_, uint64_t n) : tile_sum((n + GF_TILE - 1) / GF_TILE), tile_off((n + GF_TILE - 1) / GF_TILE + 1), off(n + 1),
		S{n, (uint32_t)((n + GF_TILE - 1) / GF_TILE), 1, tile_sum.get(), tile_off.get(), off.get()}, val{val_} {}
};
static void scan(const ScanBufs &B, unsigned grid)
{
	const GfScan &S = B.S;
	if (S.n_tiles) launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(GF_THREADS), [&] { k_ts_sums<gf_u64, TsArray<gf_u64>>(S, B.val); }, true);
	launch(dim3(1), dim3(GF_THREADS), [&] { k_ts_scan<gf_u64>(S); }, true);
	if (S.n_tiles) launch(dim3(std::min<unsigned>(grid, S.n_tiles)), dim3(GF_THREADS), [&] { k_ts_offsets<gf_u64, TsArray<gf_u64>>(S, B.val); }, true);
}
static void validate(const Case &G, JsTables &J, uint32_t flags = 0)
{
	js_validate((int64_t)G.B.size(), G.B.data(), (int64_t)G.P.size(), G.P.data(), (int64_t)G.N.size(), G.N.data(), G.cons_p.data(), G.M.data(), G.S.data(), G.D.data(), G.I.data(),
	            G.letters.data(), G.letters.size(), G.tot.data(), G.names_p.data(), G.name_len.data(), G.descs_p.data(), G.desc_len.data(), flags, J);
}

// returns false on a CHECK; throws what the host refuses (the device's refusals through js_report)
static bool emulated(const Case &G, unsigned grid, uint32_t chunk, const std::vector<uint64_t> &tile_sizes, Out &O, size_t *n_cut = nullptr)
{
	JsTables J;
	validate(G, J);
	const uint64_t nn = G.N.size(), np = G.P.size(), nb = G.B.size(), ns = J.T.n_slots, na = J.ablk.size(), n_letters = G.letters.size();
	Exact<pga_topo_node_t> nodes(nn); Exact<pga_topo_path_t> paths(np); Exact<pga_topo_block_t> blocks(nb); Exact<JsPath> meta(np);
	Exact<uint32_t> depth(nb), first(nb + 1), pathof(nn), slot_cnt(ns), blk_cnt(nb), te(TP_ERRS), ablk(na), pos(nn), order(nn), bk(nn), border(nn);
	Exact<tp_u64> key(nn); Exact<gf_u64> idk(nn), idsk(nn), jerr(JS_ERRS), cs(ns), cd(ns), ci(ns), chunks(J.n_inss), mitems(ns), bstart(na + 1), pathoff(np), tailoff(np), blockoff(nb);
	Exact<pga_rc_member_t> members(ns); Exact<pga_sub_t> subs(J.n_subs); Exact<pga_del_t> dels(J.n_dels); Exact<pga_ins_t> inss(J.n_inss); Exact<char> letters(n_letters);
	std::copy(G.N.begin(), G.N.end(), nodes.get()); std::copy(G.P.begin(), G.P.end(), paths.get()); std::copy(G.B.begin(), G.B.end(), blocks.get()); std::copy(J.meta.begin(), J.meta.end(), meta.get());
	std::copy(J.T.depth.begin(), J.T.depth.end(), depth.get()); std::copy(J.T.slot_first.begin(), J.T.slot_first.end(), first.get()); std::copy(J.ablk.begin(), J.ablk.end(), ablk.get());
	std::copy(G.M.begin(), G.M.begin() + ns, members.get()); std::copy(G.S.begin(), G.S.begin() + J.n_subs, subs.get()); std::copy(G.D.begin(), G.D.begin() + J.n_dels, dels.get());
	std::copy(G.I.begin(), G.I.begin() + J.n_inss, inss.get()); std::copy(G.letters.begin(), G.letters.end(), letters.get());
	std::fill(te.get(), te.get() + TP_ERRS, TP_NONE); std::fill(jerr.get(), jerr.get() + JS_ERRS, JS_NONE); std::fill(blockoff.get(), blockoff.get() + nb, JS_NONE);
	TpDev K;
	memset(&K, 0, sizeof(K));
	K.n_nodes = nn; K.n_paths = np; K.n_blocks = nb; K.n_slots = ns;
	K.nodes = nodes.get(); K.paths = paths.get(); K.depth = depth.get(); K.slot_first = first.get(); K.path_of = pathof.get(); K.key = key.get();
	K.slot_cnt = slot_cnt.get(); K.blk_cnt = blk_cnt.get(); K.err = te.get();
	ScanBufs b_s(cs.get(), ns), b_d(cd.get(), ns), b_i(ci.get(), ns), b_c(chunks.get(), J.n_inss), b_m(mitems.get(), ns);
	JsDev V;
	memset(&V, 0, sizeof(V));
	V.n_nodes = nn; V.n_paths = np; V.n_blocks = nb; V.n_slots = ns; V.n_alive = na; V.n_subs = J.n_subs; V.n_dels = J.n_dels; V.n_inss = J.n_inss; V.n_ins_seq = n_letters;
	V.nodes = nodes.get(); V.paths = paths.get(); V.blocks = blocks.get(); V.meta = meta.get(); V.slot_first = first.get(); V.path_of = pathof.get();
	V.members = members.get(); V.subs = subs.get(); V.dels = dels.get(); V.inss = inss.get(); V.ins_seq = letters.get(); V.chunk = chunk;
	V.id_key = idk.get(); V.pos = pos.get(); V.id_skey = idsk.get(); V.order = order.get(); V.blk_key = bk.get(); V.border = border.get(); V.err = jerr.get();
	V.cnt_s = cs.get(); V.cnt_d = cd.get(); V.cnt_i = ci.get(); V.chunks = chunks.get(); V.mitems = mitems.get(); V.ablk = ablk.get(); V.bstart = bstart.get();
	V.path_off = pathoff.get(); V.tail_off = tailoff.get(); V.block_off = blockoff.get();
	V.sub_off = b_s.S.off; V.del_off = b_d.S.off; V.ins_off = b_i.S.off; V.icoff = b_c.S.off; V.moff = b_m.S.off;
	launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_keys(K); });
	launch(dim3(grid), dim3(TP_THREADS), [&] { k_topo_check(K); });
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_idkeys(V); });
	{ std::vector<uint32_t> ix(nn); std::iota(ix.begin(), ix.end(), 0u); std::stable_sort(ix.begin(), ix.end(), [&](uint32_t a, uint32_t b) { return idk[a] < idk[b]; });
	  for (uint64_t i = 0; i < nn; ++i) { idsk[i] = idk[ix[i]]; order[i] = pos[ix[i]]; } }
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_blkkeys(V); });
	{ std::vector<uint32_t> ix(nn); std::iota(ix.begin(), ix.end(), 0u); std::stable_sort(ix.begin(), ix.end(), [&](uint32_t a, uint32_t b) { return bk[a] < bk[b]; });
	  for (uint64_t i = 0; i < nn; ++i) border[i] = order[ix[i]]; }
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_counts(V); });
	scan(b_s, grid); scan(b_d, grid); scan(b_i, grid);
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_chunks(V); });
	scan(b_c, grid);
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_check_subs(V); });
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_check_inss(V); });
	js_report(te.get(), jerr.get());
	CHECK(ns == nn);
	js_bound(J, G.B.data(), nn, b_c.off[J.n_inss], chunk);
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_mitems(V); });
	scan(b_m, grid);
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_bstart(V); });
	V.n_pitems = nn + 2 * np; V.n_bitems = 2 * na + b_m.off[ns]; V.n_items = 4 + V.n_pitems + V.n_bitems + nn;
	Exact<gf_u64> len(V.n_items);
	ScanBufs b_items(len.get(), V.n_items);
	V.len = len.get(); V.off = b_items.S.off;
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_lens(V); });
	scan(b_items, grid);
	launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_offs(V); });
	const uint64_t n_bytes = b_items.off[V.n_items];
	O.sec = {4, b_items.off[1 + V.n_pitems] + (np ? 4 : 1) + 4, b_items.off[2 + V.n_pitems + V.n_bitems] + (na ? 4 : 1) + 4};
	O.path_off.assign(pathoff.get(), pathoff.get() + np); O.block_off.assign(blockoff.get(), blockoff.get() + nb); O.order.assign(order.get(), order.get() + nn);
	js_fill_table(J, G.B.data(), G.P.data(), blockoff.get(), tailoff.get());
	// ---- the tiles, at every size asked for: the same text each time; names, descriptions and consensus letters are the host's
	std::string last;
	for (uint64_t tb : tile_sizes) {
		std::string text;
		size_t pi = 0, bi = 0;
		for (uint64_t t0 = 0; t0 < n_bytes; t0 += tb) {
			const uint64_t t1 = std::min(n_bytes, t0 + tb);
			Exact<char> tile(t1 - t0);
			memset(tile.get(), '?', t1 - t0);
			JsDev W = V;
			W.tile = tile.get(); W.t0 = t0; W.t1 = t1;
			launch(dim3(grid), dim3(GF_THREADS), [&] { k_json_tile(W); }, true);
			js_host_fill(J, G.B.data(), G.cons_p.data(), tile.get(), t0, t1, pi, bi);
			text.append(tile.get(), t1 - t0);
			if (n_cut) for (uint64_t x = 0; x < V.n_items; ++x) *n_cut += b_items.off[x] < t1 && b_items.off[x + 1] > t1;
		}
		CHECK(text.size() == n_bytes);
		CHECK(last.empty() || last == text);
		last = text;
	}
	O.text = last;
	return true;
}

static bool differ(const char *what, const std::string &a, const std::string &b)
{
	if (a == b) return false;
	size_t at = 0; while (at < a.size() && at < b.size() && a[at] == b[at]) ++at;
	fprintf(stderr, "json_emu: %s: the text differs at byte %zu of %zu / %zu (case %s)\n---- expected\n%s\n---- got\n%s\n", what, at, a.size(), b.size(), g_case.c_str(),
	        a.substr(at > 60 ? at - 60 : 0, 160).c_str(), b.substr(at > 60 ? at - 60 : 0, 160).c_str());
	return true;
}
static bool run_case(const Case &G, unsigned grid, uint32_t chunk, const std::vector<uint64_t> &tiles, size_t *n_cut = nullptr)
{
	Out E, D = direct(G);
	if (!emulated(G, grid, chunk, tiles, E, n_cut)) return false;
	if (differ("kernels against the direct construction", D.text, E.text)) return false;
	CHECK(E.sec == D.sec); CHECK(E.path_off == D.path_off); CHECK(E.block_off == D.block_off); CHECK(E.order == D.order);
	if (G.has_want) {
		if (differ("kernels against the restatement", G.want, E.text)) return false;
		CHECK(E.sec == G.want_sec); CHECK(E.path_off == G.want_path); CHECK(E.block_off == G.want_block); CHECK(E.order == G.want_order);
	}
	return true;
}

template <class F> static bool refused(F f, const char *what) { try { f(); } catch (std::runtime_error &e) { if (strstr(e.what(), what) && !strncmp(e.what(), "pga_export_json: ", 17)) return true; fprintf(stderr, "json_emu: refused with '%s', not '%s'\n", e.what(), what); return false; } fprintf(stderr, "json_emu: not refused: %s\n", what); return false; }

// two paths over three alive blocks and a dead one; slots of block 0 in descending node id; one member with every kind of edit
static Case hand_made()
{
	Case G;
	G.B = {pga_topo_block_t{5, 4, 2, 1, 0}, pga_topo_block_t{6, 9, 3, 0, 0}, pga_topo_block_t{7, 0, 1, 1, 0}, pga_topo_block_t{9, 2, 0, 1, 0}};
	G.P = {pga_topo_path_t{3, 0, 2, 1}, pga_topo_path_t{4, 2, 0, 0}, pga_topo_path_t{8, 2, 1, 0}};
	G.N = {pga_topo_node_t{30, 1, 5, 0, 0, 0, 0}, pga_topo_node_t{10, 5, 5, 2, 0, 1, 0}, pga_topo_node_t{20, 0, 4, 0, 1, 1, 0}};
	G.cons = {"ACGT", "", "", "GG"}; G.cons_null = {false, true, true, false};
	G.M = {pga_rc_member_t{1, 0, 2}, pga_rc_member_t{0, 1, 0}, pga_rc_member_t{0, 0, 0}};
	G.S = {pga_sub_t{2, 'T'}}; G.D = {pga_del_t{1, 2}}; G.I = {pga_ins_t{0, 3, 1}, pga_ins_t{4, 0, 0}}; G.letters = "xACGy";
	G.tot = {8, 0, 4}; G.names = {"a\"b", "", "c"}; G.descs = {"", "d\n", ""}; G.name_null = {false, true, false}; G.desc_null = {true, false, false};
	G.point();
	return G;
}
static const char HAND[] =
	"{\n  \"paths\": {\n    \"3\": {\n      \"id\": 3,\n      \"nodes\": [\n        30,\n        10\n      ],\n      \"tot_len\": 8,\n      \"circular\": true,\n      \"name\": \"a\\\"b\",\n"
	"      \"desc\": null\n    },\n    \"4\": {\n      \"id\": 4,\n      \"nodes\": [],\n      \"tot_len\": 0,\n      \"circular\": false,\n      \"name\": null,\n      \"desc\": \"d\\n\"\n    },\n"
	"    \"8\": {\n      \"id\": 8,\n      \"nodes\": [\n        20\n      ],\n      \"tot_len\": 4,\n      \"circular\": false,\n      \"name\": \"c\",\n      \"desc\": \"\"\n    }\n  },\n"
	"  \"blocks\": {\n    \"5\": {\n      \"id\": 5,\n      \"consensus\": \"ACGT\",\n      \"alignments\": {\n        \"20\": {\n          \"subs\": [],\n          \"dels\": [\n            {\n"
	"              \"pos\": 1,\n              \"len\": 2\n            }\n          ],\n          \"inss\": []\n        },\n        \"30\": {\n          \"subs\": [\n            {\n"
	"              \"pos\": 2,\n              \"alt\": \"T\"\n            }\n          ],\n          \"dels\": [],\n          \"inss\": [\n            {\n              \"pos\": 0,\n"
	"              \"seq\": \"ACG\"\n            },\n            {\n              \"pos\": 4,\n              \"seq\": \"\"\n            }\n          ]\n        }\n      }\n    },\n"
	"    \"7\": {\n      \"id\": 7,\n      \"consensus\": \"\",\n      \"alignments\": {\n        \"10\": {\n          \"subs\": [],\n          \"dels\": [],\n          \"inss\": []\n        }\n      }\n    },\n"
	"    \"9\": {\n      \"id\": 9,\n      \"consensus\": \"GG\",\n      \"alignments\": {}\n    }\n  },\n"
	"  \"nodes\": {\n    \"10\": {\n      \"id\": 10,\n      \"block_id\": 7,\n      \"path_id\": 3,\n      \"strand\": \"-\",\n      \"position\": [\n        5,\n        5\n      ]\n    },\n"
	"    \"20\": {\n      \"id\": 20,\n      \"block_id\": 5,\n      \"path_id\": 8,\n      \"strand\": \"-\",\n      \"position\": [\n        0,\n        4\n      ]\n    },\n"
	"    \"30\": {\n      \"id\": 30,\n      \"block_id\": 5,\n      \"path_id\": 3,\n      \"strand\": \"+\",\n      \"position\": [\n        1,\n        5\n      ]\n    }\n  }\n}";

int main(int argc, char **argv)
{
	size_t n_cut = 0;
	// ---- the hand-made graph: the text written out, tiles from 7 bytes up, chunks of 1, 2 and 64 letters
	const Case H = hand_made();
	{
		Out E;
		if (!emulated(H, 2, 2, {7, 64, 4096}, E, &n_cut)) return 1;
		if (differ("the hand-made graph", HAND, E.text)) return 1;
		for (uint32_t chunk : {1u, 64u}) if (!run_case(H, 1, chunk, {13, 1000})) return 1;
		if (E.order != std::vector<uint32_t>{1, 2, 0} || E.block_off[1] != JS_NONE || E.text.compare(E.block_off[2], 6, "\"7\": {") || E.text.compare(E.path_off[1], 6, "\"4\": {") ||
		    E.text.compare(E.sec[2], 7, "\"nodes\"")) { fprintf(stderr, "json_emu: the tables of the hand-made graph are off\n"); return 1; }
	}
	// ---- the named cases of tests/json_gen.py
	for (int a = 1; a < argc; ++a) {
		Case G;
		g_case = argv[a];
		if (!load(argv[a], G)) { fprintf(stderr, "json_emu: cannot read %s\n", argv[a]); return 1; }
		const bool big = G.want.size() > 60000;
		std::vector<uint64_t> tiles{std::max<uint64_t>(251, G.want.size() / 6 | 1)};                 // a handful of tiles of an odd size
		if (!big && G.want.size() > 4096) tiles.push_back(4096);
		if (!run_case(G, big ? 3 : 1 + a % 2, JS_CHUNK, tiles, &n_cut)) return 1;
		if (!big && !G.I.empty() && !run_case(G, 2, 5, {1000003})) return 1;                         // another chunk: the same text
	}
	g_case = "built-in";
	if (n_cut < 40) { fprintf(stderr, "json_emu: only %zu items were cut by a tile edge\n", n_cut); return 1; }
	// ---- escaping: every byte, against the direct formatter
	for (int c = 0; c < 256; ++c) {
		const char s[3] = {'x', (char)c, 'y'};
		Pretty W; W.str(std::string(s, 3));
		if ('"' + js_escape(s, 3) + '"' != W.s) { fprintf(stderr, "json_emu: byte %d is escaped differently\n", c); return 1; }
	}
	if (js_escape("\x01\x1f\x7f\n", 4) != "\\u0001\\u001f\x7f\\n" || sizeof(JS_EMPTY) - 1 != strlen("{\n  \"paths\": {},\n  \"blocks\": {},\n  \"nodes\": {}\n}")) return 1;
	{ Pretty W; W.begin('{'); for (const char *k : {"paths", "blocks", "nodes"}) { W.key(k); W.begin('{'); W.end('}'); } W.end('}'); if (W.s != JS_EMPTY) return 1; }
	// ---- what is refused: on the host, and by the kernels before an index is derived
	bool ok = true;
	auto host = [&](const Case &X, uint32_t flags = 0) { JsTables J; validate(X, J, flags); };
	auto device = [&](const Case &X) { Out E; emulated(X, 2, JS_CHUNK, {512}, E); };
	host(H);
	Case X = H; X.N[0].member = 2;                      ok = ok && refused([&] { host(X); }, "member >= depth");
	X = H; X.N[0].block = 1;                            ok = ok && refused([&] { host(X); }, "dead block");
	X = H; X.P[2].node_off = 1;                         ok = ok && refused([&] { host(X); }, "node_off is not the running sum");
	X = H; X.P[1].path_id = 3;                          ok = ok && refused([&] { host(X); }, "path ids are not ascending");
	X = H; X.B[2].block_id = 5;                         ok = ok && refused([&] { host(X); }, "not strictly ascending");
	ok = ok && refused([&] { host(H, 1); }, "unknown flag");
	X = H; X.cons_p[0] = nullptr;                       ok = ok && refused([&] { host(X); }, "null consensus of an alive block (block 0)");
	X = H; X.cons_p[2] = nullptr; host(X);                                                           // (an empty consensus is not read)
	{ JsTables J; ok = ok && refused([&] { js_validate(4, H.B.data(), 3, H.P.data(), 3, H.N.data(), H.cons_p.data(), nullptr, H.S.data(), H.D.data(), H.I.data(), H.letters.data(), 5, H.tot.data(), H.names_p.data(), H.name_len.data(), H.descs_p.data(), H.desc_len.data(), 0, J); }, "null members"); }
	{ JsTables J; ok = ok && refused([&] { js_validate(4, H.B.data(), 3, H.P.data(), 3, H.N.data(), H.cons_p.data(), H.M.data(), H.S.data(), nullptr, H.I.data(), H.letters.data(), 5, H.tot.data(), H.names_p.data(), H.name_len.data(), H.descs_p.data(), H.desc_len.data(), 0, J); }, "null edit list"); }
	{ JsTables J; ok = ok && refused([&] { js_validate(4, H.B.data(), 3, H.P.data(), 3, H.N.data(), H.cons_p.data(), H.M.data(), H.S.data(), H.D.data(), H.I.data(), nullptr, 5, H.tot.data(), H.names_p.data(), H.name_len.data(), H.descs_p.data(), H.desc_len.data(), 0, J); }, "null insertion letters"); }
	{ JsTables J; ok = ok && refused([&] { js_validate(4, H.B.data(), 3, H.P.data(), 3, H.N.data(), H.cons_p.data(), H.M.data(), H.S.data(), H.D.data(), H.I.data(), H.letters.data(), 5, nullptr, H.names_p.data(), H.name_len.data(), H.descs_p.data(), H.desc_len.data(), 0, J); }, "null tot_len, names or descs"); }
	{ JsTables J; ok = ok && refused([&] { js_validate(4, H.B.data(), 3, H.P.data(), 3, H.N.data(), H.cons_p.data(), H.M.data(), H.S.data(), H.D.data(), H.I.data(), H.letters.data(), 5, H.tot.data(), H.names_p.data(), H.name_len.data(), nullptr, H.desc_len.data(), 0, J); }, "null tot_len, names or descs"); }
	if (!ok) { fprintf(stderr, "json_emu: a refusal of the host is off\n"); return 1; }
	X = H; X.N[2].member = 0;                           ok = ok && refused([&] { device(X); }, "slot is named by two nodes");
	X = H; X.N[2].node_id = 30;                         ok = ok && refused([&] { device(X); }, "two nodes with one node_id");
	X = H; X.N[1].node_id = 30;                         ok = ok && refused([&] { device(X); }, "two nodes with one node_id");   // (in two blocks)
	for (uint32_t bad : {0x1fu, 0x7fu, (uint32_t)'"', (uint32_t)'\\', 0x141u}) { X = H; X.S[0].alt = bad; ok = ok && refused([&] { device(X); }, "a substitution letter that JSON would escape (sub 0)"); }
	X = H; X.I[0].seq_off = 3;                          ok = ok && refused([&] { device(X); }, "runs past the insertion letters (insertion 0)");
	X = H; X.I[1].seq_off = 6;                          ok = ok && refused([&] { device(X); }, "runs past the insertion letters (insertion 1)");
	X = H; X.I[0].len = 0xffffffffu;                    ok = ok && refused([&] { device(X); }, "runs past the insertion letters (insertion 0)");
	X = H; X.I[0].seq_off = ~0ULL;                      ok = ok && refused([&] { device(X); }, "runs past the insertion letters (insertion 0)");
	for (char bad : {'\n', '"', '\\', '\x7f', '\xc3'}) { X = H; X.letters[2] = bad; ok = ok && refused([&] { device(X); }, "an insertion letter that JSON would escape (insertion 0)"); }
	X = H; X.letters[0] = '\n'; X.letters[4] = '"'; device(X);                                       // (letters no insertion names are not read)
	if (!ok) { fprintf(stderr, "json_emu: a refusal of the kernels is off\n"); return 1; }
	{ JsTables J; validate(H, J); ok = ok && refused([&] { js_bound(J, H.B.data(), 3, 1ULL << 58, 64); }, "a file of 2^63 bytes or more"); js_bound(J, H.B.data(), 3, 1ULL << 56, 64); }
	if (!ok) return 1;
	printf("json_emu OK (%d cases from files, %zu items cut by a tile edge)\n", argc - 1, n_cut);
	return 0;
}
