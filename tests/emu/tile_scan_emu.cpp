// pga_tile_scan.h without a device and on its own: the three kernels under dev/emu/hip_emu.h for both word types, with every buffer
// allocated at exactly the size the kernels may touch (under the address sanitizer an access one entry out is an error), against a scalar
// prefix sum; then the second level fed directly with more tile sums than the one workgroup has threads.
// Build and run (host only):  g++ -std=c++17 -g -O1 -DPGA_EMU -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined
//                             tests/emu/tile_scan_emu.cpp -o tile_scan_emu && ./tile_scan_emu
#include <cstdio>
#include <memory>
#include <random>
#include "../../dev/emu/hip_emu.h"
#include "../../pangraph_amd/csrc/pga_tile_scan.h"

using namespace pga;

template <class T> struct Exact {                                       // n entries, not one more
	std::unique_ptr<T[]> p; size_t n;
	explicit Exact(size_t n_) : p(n_ ? new T[n_]() : nullptr), n(n_) {}
	T *get() { return p.get(); }
	T &operator[](size_t i) { return p[i]; }
};

static std::mt19937 rng(20261020);
static uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0u; }
// a 64-bit value needs its upper half now and then; the 32-bit sums stay below 2^32 at every size used here
template <class T> static T value() { return sizeof(T) == 8 ? (rnd(5) ? (T)rnd(1000) : (T)((ts_u64)rng() << 8)) : (T)rnd(1000); }

// n_q quantities side by side, quantity q of item i at val[q * n + i]
template <class T> struct ValRows { const T *val; ts_u64 n; T operator()(int q, uint64_t i) const { return val[(size_t)q * n + i]; } };

template <class T> static bool whole_scan(uint64_t n, uint32_t n_q, unsigned grid_kind)
{
	const uint32_t n_tiles = (uint32_t)((n + TS_TILE - 1) / TS_TILE);
	const unsigned grid = grid_kind == 0 ? 1 : grid_kind == 1 ? 2 : n_tiles;
	Exact<T> val((size_t)n_q * n), sums((size_t)n_q * n_tiles), offs((size_t)n_q * (n_tiles + 1)), off((size_t)n_q * (n + 1));
	for (size_t i = 0; i < val.n; ++i) val[i] = value<T>();
	const TileScan<T> S{n, n_tiles, n_q, sums.get(), offs.get(), off.get()};
	const ValRows<T> V{val.get(), n};
	if (n_tiles) emu_launch(dim3(std::min<unsigned>(grid, n_tiles)), dim3(TS_THREADS), [&] { k_ts_sums<T, ValRows<T>>(S, V); });
	emu_launch(dim3(1), dim3(TS_THREADS), [&] { k_ts_scan<T>(S); });
	if (n_tiles) emu_launch(dim3(std::min<unsigned>(grid, n_tiles)), dim3(TS_THREADS), [&] { k_ts_offsets<T, ValRows<T>>(S, V); });
	for (uint32_t q = 0; q < n_q; ++q) {
		T run = 0, tile = 0;
		for (uint64_t i = 0; i <= n; ++i) {
			if (i % TS_TILE == 0 && i < n && offs[(size_t)q * (n_tiles + 1) + i / TS_TILE] != run) return false;
			if (i % TS_TILE == 0 && i) { if (sums[(size_t)q * n_tiles + i / TS_TILE - 1] != tile) return false; tile = 0; }
			if (ts_off(S, (int)q)[i] != run) return false;
			if (i < n) { run += val[(size_t)q * n + i]; tile += val[(size_t)q * n + i]; }
		}
		if (n % TS_TILE && sums[(size_t)q * n_tiles + n_tiles - 1] != tile) return false;
		if (offs[(size_t)q * (n_tiles + 1) + n_tiles] != run) return false;
	}
	return true;
}

// the second level of the tile scan on its own: more tile sums than the one workgroup has threads, n_q quantities
template <class T, class Make> static bool second_level(uint32_t n_q, Make make)
{
	const uint32_t n_tiles = 2 * TS_THREADS + 3;
	Exact<T> sums(n_q * (size_t)n_tiles), offs(n_q * ((size_t)n_tiles + 1)), off(n_q * (size_t)2);
	for (size_t i = 0; i < sums.n; ++i) sums[i] = make();
	const TileScan<T> S{1, n_tiles, n_q, sums.get(), offs.get(), off.get()};                    // (n: only where the totals go)
	emu_launch(dim3(1), dim3(TS_THREADS), [&] { k_ts_scan<T>(S); });
	for (uint32_t q = 0; q < n_q; ++q) {
		T run = 0;
		for (uint32_t t = 0; t <= n_tiles; ++t) { if (offs[(size_t)q * (n_tiles + 1) + t] != run) { fprintf(stderr, "tile_scan_emu: the tile scan is off at tile %u\n", t); return false; } if (t < n_tiles) run += sums[(size_t)q * n_tiles + t]; }
		if (off[q * 2 + 1] != run) { fprintf(stderr, "tile_scan_emu: the tile scan's total is off\n"); return false; }
	}
	return true;
}

// Every small size with every number of quantities and every grid; the size that needs the second level's loop (more than TS_THREADS
// tiles) costs the emulator seconds per quantity, so it runs with one quantity: both grid extremes in 64 bits, the middle one in 32
// (seven quantities over more than TS_THREADS tiles are second_level's below).
template <class T> static bool word_type(const char *name)
{
	const uint64_t sizes[] = {0, 1, 1023, 1024, 1025, 3 * 1024 + 5, 1024 * 256 + 1};
	for (uint64_t n : sizes) for (uint32_t n_q : {1u, 7u}) for (unsigned g = 0; g < 3; ++g) {
		if (n > 4 * TS_TILE && (n_q != 1 || (sizeof(T) == 8) == (g == 1))) continue;
		if (!whole_scan<T>(n, n_q, g)) { fprintf(stderr, "tile_scan_emu: %s: the scan of %llu items, %u quantities, grid kind %u is off\n", name, (unsigned long long)n, n_q, g); return false; }
	}
	return true;
}

int main()
{
	if (!word_type<uint32_t>("32 bits") || !word_type<ts_u64>("64 bits")) return 1;
	// as the entries that use the scan fed it: two and three quantities with values up to 2^40, one quantity with values up to 2^20
	if (!second_level<ts_u64>(2, [] { return rnd(5) ? rnd(1000) : (ts_u64)rng() << 8; })) return 1;
	if (!second_level<ts_u64>(3, [] { return rnd(5) ? rnd(1000) : (ts_u64)rng() << 8; })) return 1;
	if (!second_level<ts_u64>(1, [] { return rnd(5) ? rnd(1000) : (ts_u64)rng() >> 12; })) return 1;
	if (!second_level<uint32_t>(7, [] { return rnd(1000); })) return 1;
	const ts_u64 offs[6] = {0, 2, 2, 2, 5, 5};
	if (ts_last_le(offs, 0, 5, 0) != 0 || ts_last_le(offs, 0, 5, 1) != 0 || ts_last_le(offs, 0, 5, 2) != 3 || ts_last_le(offs, 0, 5, 4) != 3 || ts_last_le(offs, 3, 4, 4) != 3) { fprintf(stderr, "tile_scan_emu: a lookup is off\n"); return 1; }
	printf("tile_scan_emu OK\n");
	return 0;
}
