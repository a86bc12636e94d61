// pga_tile_scan.h -- the two-level exclusive scan of the graph entries, once: a workgroup scan through LDS per tile of TS_TILE items, the
// tile sums, ONE workgroup over the tile sums, then every item's offset.  Several quantities are scanned side by side (n_q of them, each
// with its own row of every buffer); what an item is worth comes from a functor, so no entry keeps a copy of the three kernels.
// No wave intrinsic, barriers only: all of this compiles under hipcc and, with dev/emu/hip_emu.h included first, under
// g++ -std=c++17 -DPGA_EMU (tests/emu/tile_scan_emu.cpp runs it against a scalar prefix sum); the host side needs HIP and is left out there.
// pga_topo_idx.h keeps its own fused consumer of the tile offsets (k_topo_splice) and takes only ts_block_excl from here.
#pragma once
#ifndef PGA_EMU
#include "pga_common.h"
#endif
#include <algorithm>
#include <stdint.h>

namespace pga {

typedef unsigned long long ts_u64;
constexpr int TS_THREADS = 256, TS_ITEMS = 4, TS_TILE = TS_THREADS * TS_ITEMS;

// exclusive sums of one value per thread over the workgroup, through LDS (s: TS_THREADS entries); total: the workgroup's sum
template <class T> __device__ inline T ts_block_excl(T v, T *s, T &total)
{
	const uint32_t t = threadIdx.x;
	s[t] = v;
	__syncthreads();
	for (uint32_t d = 1; d < (uint32_t)TS_THREADS; d <<= 1) {
		const T x = t >= d ? s[t - d] : (T)0;
		__syncthreads();
		s[t] += x;
		__syncthreads();
	}
	total = s[TS_THREADS - 1];
	const T before = s[t] - v;
	__syncthreads();
	return before;
}

// one scan: n items, n_q quantities; tile_sum: n_q x n_tiles; tile_off: n_q x (n_tiles + 1); off: n_q x (n + 1), off[q][n] the total
template <class T> struct TileScan { ts_u64 n; uint32_t n_tiles, n_q; T *tile_sum, *tile_off, *off; };
template <class T> __host__ __device__ inline const T *ts_off(const TileScan<T> &S, int q) { return S.off + (ts_u64)q * (S.n + 1); }
// the last index x in [lo, hi) with off[x] <= j, given off[lo] <= j < off[hi]: the item that holds element j (empty items share their
// offset with the item behind them)
__host__ __device__ inline ts_u64 ts_last_le(const ts_u64 *off, ts_u64 lo, ts_u64 hi, ts_u64 j)
{
	while (hi - lo > 1) { const ts_u64 mid = (lo + hi) >> 1; if (off[mid] <= j) lo = mid; else hi = mid; }
	return lo;
}
// A value functor is small and trivially copyable, `T operator()(int q, uint64_t i) const`, and goes to the kernels by value.
// The plainest one: one quantity, read from an array
template <class T> struct TsArray { const T *val; __host__ __device__ T operator()(int, uint64_t i) const { return val[i]; } };

template <class T, class Val> static __global__ __launch_bounds__(TS_THREADS) void k_ts_sums(TileScan<T> S, Val val)
{
	__shared__ T s[TS_THREADS];
	for (uint32_t t = blockIdx.x; t < S.n_tiles; t += gridDim.x) {
		const ts_u64 i0 = (ts_u64)t * TS_TILE + (ts_u64)threadIdx.x * TS_ITEMS;
		for (uint32_t q = 0; q < S.n_q; ++q) {
			T v = 0, total;
			for (int k = 0; k < TS_ITEMS; ++k) if (i0 + k < S.n) v += val((int)q, i0 + k);
			ts_block_excl(v, s, total);
			if (threadIdx.x == 0) S.tile_sum[(ts_u64)q * S.n_tiles + t] = total;
		}
	}
}
// ONE workgroup: tile_off[q][t] = what the tiles before t add; tile_off[q][n_tiles] = off[q][n] = the total
template <class T> static __global__ __launch_bounds__(TS_THREADS) void k_ts_scan(TileScan<T> S)
{
	__shared__ T s[TS_THREADS];
	for (uint32_t q = 0; q < S.n_q; ++q) {
		T run = 0;
		for (uint32_t t0 = 0; t0 < S.n_tiles; t0 += TS_THREADS) {
			const uint32_t t = t0 + threadIdx.x;
			const T v = t < S.n_tiles ? S.tile_sum[(ts_u64)q * S.n_tiles + t] : (T)0;
			T total;
			const T before = ts_block_excl(v, s, total);
			if (t < S.n_tiles) S.tile_off[(ts_u64)q * (S.n_tiles + 1) + t] = run + before;
			run += total;
		}
		if (threadIdx.x == 0) { S.tile_off[(ts_u64)q * (S.n_tiles + 1) + S.n_tiles] = run; S.off[(ts_u64)q * (S.n + 1) + S.n] = run; }
	}
}
template <class T, class Val> static __global__ __launch_bounds__(TS_THREADS) void k_ts_offsets(TileScan<T> S, Val val)
{
	__shared__ T s[TS_THREADS];
	for (uint32_t t = blockIdx.x; t < S.n_tiles; t += gridDim.x) {
		const ts_u64 i0 = (ts_u64)t * TS_TILE + (ts_u64)threadIdx.x * TS_ITEMS;
		for (uint32_t q = 0; q < S.n_q; ++q) {
			T c[TS_ITEMS], v = 0, total;
			for (int k = 0; k < TS_ITEMS; ++k) { c[k] = i0 + k < S.n ? val((int)q, i0 + k) : (T)0; v += c[k]; }
			T at = S.tile_off[(ts_u64)q * (S.n_tiles + 1) + t] + ts_block_excl(v, s, total);
			for (int k = 0; k < TS_ITEMS && i0 + k < S.n; ++k) { S.off[(ts_u64)q * (S.n + 1) + i0 + k] = at; at += c[k]; }
		}
	}
}

#ifndef PGA_EMU
// the scan's buffers: every one an entry longer than its count, none is empty
template <class T> struct TileScanBufs {
	DBuf<T> tile_sum, tile_off, off;
	TileScan<T> make(uint64_t n, uint32_t n_q)
	{
		const uint32_t n_tiles = (uint32_t)((n + TS_TILE - 1) / TS_TILE);
		tile_sum.alloc((uint64_t)n_q * n_tiles + 1); tile_off.alloc((uint64_t)n_q * (n_tiles + 1)); off.alloc((uint64_t)n_q * (n + 1));
		return TileScan<T>{n, n_tiles, n_q, tile_sum.p, tile_off.p, off.p};
	}
};
template <class T, class Val> inline void tile_scan_launch(const TileScan<T> &S, Val val, hipStream_t st)
{
	const dim3 grid(std::min<uint32_t>(S.n_tiles, 2048u));
	if (S.n_tiles) hipLaunchKernelGGL((k_ts_sums<T, Val>), grid, dim3(TS_THREADS), 0, st, S, val);
	hipLaunchKernelGGL(k_ts_scan<T>, dim3(1), dim3(TS_THREADS), 0, st, S);
	if (S.n_tiles) hipLaunchKernelGGL((k_ts_offsets<T, Val>), grid, dim3(TS_THREADS), 0, st, S, val);
}
#endif

} // namespace pga
