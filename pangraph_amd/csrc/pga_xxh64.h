// pga_xxh64.h -- XXH64, the hash behind every id of the graph (utils/id.rs: seed 0 over little-endian words and letters), once.
// xxh64_words runs on the host and on the device; with a constant n its loops unroll and the word array stays in registers.
// Compiles under hipcc and, with dev/emu/hip_emu.h included first, under g++ -std=c++17 -DPGA_EMU.
#pragma once
#include <stdint.h>

namespace pga {

__host__ __device__ inline uint64_t xxh64_rol(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
// seed 0, n little-endian u64 words
__host__ __device__ inline uint64_t xxh64_words(const uint64_t *w, int n)
{
	const uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL, P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
	uint64_t h; int at = 0;
	if (n >= 4) {
		uint64_t v0 = P1 + P2, v1 = P2, v2 = 0, v3 = 0 - P1;
		for (; n - at >= 4; at += 4) {
			v0 = xxh64_rol(v0 + w[at] * P2, 31) * P1; v1 = xxh64_rol(v1 + w[at + 1] * P2, 31) * P1;
			v2 = xxh64_rol(v2 + w[at + 2] * P2, 31) * P1; v3 = xxh64_rol(v3 + w[at + 3] * P2, 31) * P1;
		}
		h = xxh64_rol(v0, 1) + xxh64_rol(v1, 7) + xxh64_rol(v2, 12) + xxh64_rol(v3, 18);
		h = (h ^ (xxh64_rol(v0 * P2, 31) * P1)) * P1 + P4; h = (h ^ (xxh64_rol(v1 * P2, 31) * P1)) * P1 + P4;
		h = (h ^ (xxh64_rol(v2 * P2, 31) * P1)) * P1 + P4; h = (h ^ (xxh64_rol(v3 * P2, 31) * P1)) * P1 + P4;
	} else h = P5;
	h += (uint64_t)n * 8;
	for (; at < n; ++at) h = xxh64_rol(h ^ (xxh64_rol(w[at] * P2, 31) * P1), 27) * P1 + P4;
	h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
	return h;
}
// n bytes, host only
inline uint64_t xxh64_bytes(const uint8_t *p, uint64_t n, uint64_t seed)
{
	const uint64_t P1 = 0x9E3779B185EBCA87ULL, P2 = 0xC2B2AE3D27D4EB4FULL, P3 = 0x165667B19E3779F9ULL, P4 = 0x85EBCA77C2B2AE63ULL, P5 = 0x27D4EB2F165667C5ULL;
	auto rd64 = [](const uint8_t *q) { uint64_t v = 0; for (int i = 7; i >= 0; --i) v = v << 8 | q[i]; return v; };
	auto round = [&](uint64_t acc, uint64_t in) { return xxh64_rol(acc + in * P2, 31) * P1; };
	const uint8_t *end = p + n;
	uint64_t h;
	if (n >= 32) {
		uint64_t v[4] = {seed + P1 + P2, seed + P2, seed, seed - P1};
		for (; end - p >= 32; p += 32) for (int i = 0; i < 4; ++i) v[i] = round(v[i], rd64(p + 8 * i));
		h = xxh64_rol(v[0], 1) + xxh64_rol(v[1], 7) + xxh64_rol(v[2], 12) + xxh64_rol(v[3], 18);
		for (int i = 0; i < 4; ++i) h = (h ^ round(0, v[i])) * P1 + P4;
	} else h = seed + P5;
	h += n;
	for (; end - p >= 8; p += 8) h = xxh64_rol(h ^ round(0, rd64(p)), 27) * P1 + P4;
	if (end - p >= 4) { const uint64_t w = (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24; h = xxh64_rol(h ^ (w * P1), 23) * P2 + P3; p += 4; }
	for (; p < end; ++p) h = xxh64_rol(h ^ (*p * P5), 11) * P1;
	h ^= h >> 33; h *= P2; h ^= h >> 29; h *= P3; h ^= h >> 32;
	return h;
}

} // namespace pga
