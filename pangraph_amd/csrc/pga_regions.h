// pga_regions.h -- region records of a query from its chains, and their ranking: the host restatement of hit.c's bookkeeping and of the mapq /
// rescale arithmetic (pga_regions.cpp).  Pure host code over compact records: no device state, no bases.
#pragma once
#include "pga_pipeline.h"
#include "pga_plan.h"

namespace pga {

inline uint32_t name_hash31(const std::string &s) { uint32_t h = 0; bool first = true; for (unsigned char c : s) { h = first ? c : h * 31u + c; first = false; } return h; }   // X31 string hash (khash.h)
inline uint32_t mix32(uint32_t k) { k += ~(k << 15); k ^= k >> 10; k += k << 3; k ^= k >> 6; k += ~(k << 11); k ^= k >> 16; return k; }   // Wang's 32-bit mix (map.c:246-248)

// One region per chain, ordered by descending (score<<32 | cnt) ^ salt(first anchor, query) -- hit.c:52-88.
// heads: the first anchor of every chain, gathered on the device (then A holds no anchors and the extents are left to the planner)
void regions_from_chains(uint32_t query_salt, int qlen, int n_chains, const uint64_t *u, const Anchors &A, std::vector<Reg> &regs, const u128 *heads = nullptr);
// The tail of `head` from its anchor `n_keep` on becomes its own region (hit.c:106-123); extents = false: the planner fills them in
void cut_region(Reg &head, Reg &tail, int n_keep, int qlen, const Anchors &A, bool extents = true);
void drop_weak_regions(const mm_mapopt_t &opt, int qlen, std::vector<Reg> &regs);                 // hit.c:290-309
void order_regions(std::vector<Reg> &regs);                                                        // hit.c:188-218
void assign_mapq(std::vector<Reg> &regs, int min_chain_sc, int match_sc, int rep_len);            // hit.c:396-466
void rescale_dp_max(int qlen, std::vector<Reg> &regs, float frac, int a, int b);                  // align.c:897-960

} // namespace pga
