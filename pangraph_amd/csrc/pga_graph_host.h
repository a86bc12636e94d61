// pga_graph_host.h -- what the hosts of the graph entries (pga_slice.hip ... pga_json.hip) share beside DBuf / Downloads / StreamLease of
// pga_common.h: the output arrays, the grids, the guarded copies, events and pinned blocks, the clocks, the two-call rocPRIM wrappers
// and the tile knob of the exports.  Host code only.
#pragma once
#include "pga_common.h"
#include <chrono>
#include <rocprim/rocprim.hpp>

namespace pga {

// an output array of the C ABI (the caller frees it): zeroed, never NULL; entry: the name the refusal carries
template <class T> inline T *host_array(uint64_t n, const char *entry)
{
	T *p = (T*)calloc((size_t)(n ? n : 1), sizeof(T));
	if (!p) throw std::runtime_error(std::string(entry) + ": out of host memory");
	return p;
}
// workgroups for `items` at per_block each: at least one, at most cap
inline unsigned grid_for(uint64_t items, uint64_t per_block, uint64_t cap) { return (unsigned)std::min<uint64_t>(std::max<uint64_t>((items + per_block - 1) / per_block, 1), cap); }
template <class T> inline void upload(DBuf<T> &d, const T *h, uint64_t n, hipStream_t st) { if (n) PGA_HIP(hipMemcpyAsync(d.p, h, n * sizeof(T), hipMemcpyHostToDevice, st)); }
template <class T> inline void fetch(T *dst, const T *src, uint64_t n, hipStream_t st) { if (n) PGA_HIP(hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, st)); }

struct Event { hipEvent_t e = nullptr; Event() { PGA_HIP(hipEventCreate(&e)); } ~Event() { (void)hipEventDestroy(e); } };
struct PinBlock { char *p = nullptr; ~PinBlock() { pin_free(p); } };
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
// the stream's clock at four places of a call: upload, kernels (their waits included), download, in ms
struct StageClock {
	hipEvent_t e[4]; hipStream_t st;
	explicit StageClock(hipStream_t s) : st(s) { for (hipEvent_t &x : e) PGA_HIP(hipEventCreate(&x)); }
	void at(int i) { PGA_HIP(hipEventRecord(e[i], st)); }
	void read(double *ms3) { for (int i = 0; i < 3; ++i) { float ms = 0; PGA_HIP(hipEventElapsedTime(&ms, e[i], e[i + 1])); ms3[i] = ms; } }
	~StageClock() { for (hipEvent_t &x : e) (void)hipEventDestroy(x); }
};

// rocPRIM in two calls: the size of the temporary storage, then the work
template <class K> inline void radix_sort_keys(const K *in, K *out, uint64_t n, unsigned bits, hipStream_t st)
{
	size_t tb = 0;
	PGA_HIP(rocprim::radix_sort_keys(nullptr, tb, in, out, n, 0, bits, st));
	DBuf<uint8_t> tmp(tb + 16);
	PGA_HIP(rocprim::radix_sort_keys(tmp.p, tb, in, out, n, 0, bits, st));
}
template <class K> inline void radix_sort_pairs(const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, uint64_t n, unsigned bits, hipStream_t st)
{
	if (!n) return;
	size_t tb = 0;
	PGA_HIP(rocprim::radix_sort_pairs(nullptr, tb, kin, kout, vin, vout, n, 0, bits, st));
	DBuf<uint8_t> tmp(tb + 16);
	PGA_HIP(rocprim::radix_sort_pairs(tmp.p, tb, kin, kout, vin, vout, n, 0, bits, st));
}
template <class T> inline void excl_scan(const T *in, T *out, size_t n, hipStream_t st)
{
	size_t tb = 0;
	PGA_HIP(rocprim::exclusive_scan(nullptr, tb, in, out, (T)0, n, rocprim::plus<T>(), st));
	DBuf<uint8_t> tmp(tb + 16);
	PGA_HIP(rocprim::exclusive_scan(tmp.p, tb, in, out, (T)0, n, rocprim::plus<T>(), st));
}

// an environment knob in KB, read at every call; fail(what) throws with the entry's name in front
template <class Fail> inline uint64_t knob_kb(Fail fail, const char *name, uint64_t dflt, uint64_t multiple)
{
	const char *e = getenv(name);
	if (!e || !*e) return dflt;
	char *end = nullptr;
	const long long v = strtoll(e, &end, 10);
	if (*end || v < (long long)multiple || v > (1LL << 31) || (uint64_t)v % multiple)
		fail(std::string(name) + " must be a whole number of KB, a multiple of " + std::to_string(multiple) + " (got '" + e + "')");
	return (uint64_t)v;
}
// PGA_EXPORT_TILE_KB: the bytes of an export's tile
template <class Fail> inline uint64_t export_tile_bytes(Fail fail) { return knob_kb(fail, "PGA_EXPORT_TILE_KB", 16384, 4) * 1024; }

} // namespace pga
