// gg_modep_mt.h — miss-type tracking of the private (Mode P) replay and the
// Cache quartet: Cache::getMissType / updateMissCounters /
// clearMissTypeTrackingSets (cache.cc:28-40,131-148,228-230,321-405) over the
// evicted / invalidated / fetched address sets of every tracked cache.
//
// Table: [tile][tracked cache][L1-D set][slot], lines / u1 slots of 8 B per
// (tile, cache, L1-D set), contiguous, so a linear probe walks 64-B lines.  One
// word per line: line byte address | bits (evicted 1, invalidated 2, fetched 4),
// ~0 = empty (the coherent table's word format, gg_coh_dev.h).  A line belongs
// to exactly one replay unit (tile, L1-D set) in both caches, and a unit is
// owned by one lane (streaming and sharded replay) or by the single quartet
// thread, stream-ordered with the batches: no atomics, no cross-lane protocol.
// The hash takes the line bits above the L1-D set index (the low bits are the
// same for every line of a unit).
//
// Capacity rule: lines are never removed, so a slice holds every distinct
// line its unit ever installed; a run fails (GG_DERR_MT_CAP) exactly when
// some unit has to hold more distinct lines than lines / u1.  Both caches of a
// tile see the same lines, so one rule covers both.  Every probe loop is
// bounded by the slot count; a full slice sets the error bit and writes
// nothing.
#pragma once
#include "gg_internal.h"

// One cache's slice of one unit.
struct gg_mt_set {
  uint64_t* s;          // the unit's slots (nullptr: this cache is not tracked)
  uint32_t mask;        // slots - 1
  uint32_t log_line;
  uint32_t hshift;      // 64 - log2(slots)
  uint32_t log_u1;
  static constexpr uint64_t kEmpty = ~0ull;
  static constexpr uint32_t kE = 1, kI = 2, kF = 4;

  __device__ __forceinline__ bool on() const { return s != nullptr; }

  // Slot of byte address `a` (its word, or the first empty slot of its probe
  // sequence) and the line's bits; ~0u with the error bit when the slice is
  // full and does not hold the line.
  __device__ __forceinline__ uint32_t slot(uint64_t a, uint32_t& bits, uint32_t& err) const
  {
    const uint32_t h = (uint32_t)((((a >> log_line) >> log_u1) * 0x9E3779B97F4A7C15ull) >> hshift);
    for (uint32_t n = 0; n <= mask; ++n) {
      const uint32_t i = (h + n) & mask;
      const uint64_t k = s[i];
      if (k == kEmpty) { bits = 0; return i; }
      if ((k & ~7ull) == a) { bits = (uint32_t)k & 7u; return i; }
    }
    err |= GG_DERR_MT_CAP;
    bits = 0;
    return ~0u;
  }
  // A lane's later probes must see this word: wait for the store (as the
  // coherent table's mt_put does).  Full slice: flagged, no slot overwritten.
  __device__ __forceinline__ void put(uint32_t i, uint64_t a, uint32_t bits) const
  {
    if (i == ~0u) return;
    s[i] = a | bits;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  // setCacheLineInfo(INVALID) (cache.cc:228-230) / the victim of an insert
  __device__ __forceinline__ void or_bits(uint64_t a, uint32_t b, uint32_t& err) const
  {
    uint32_t bits;
    const uint32_t i = slot(a, bits, err);
    if ((bits & b) != b) put(i, a, bits | b);
  }
  // insertCacheLine (cache.cc:131-148): the victim into the evicted set; the
  // inserted line out of the first set that holds it
  // (clearMissTypeTrackingSets, :398-404), then into the fetched set
  __device__ __forceinline__ void insert(uint64_t a, bool ev, uint64_t ev_addr, uint32_t& err) const
  {
    if (ev) or_bits(ev_addr, kE, err);
    uint32_t bits;
    const uint32_t i = slot(a, bits, err);
    uint32_t nb = bits;
    if (nb & kE) nb &= ~kE;
    else if (nb & kI) nb &= ~kI;
    else if (nb & kF) nb &= ~kF;
    nb |= kF;
    if (nb != bits) put(i, a, nb);          // (a held word never has bits == 0)
  }
  // getMissType (cache.cc:363-375): GG_MT_*
  __device__ __forceinline__ uint32_t classify(uint64_t a, uint32_t& err) const
  {
    uint32_t bits;
    (void)slot(a, bits, err);
    return (bits & kE) ? GG_MT_CAPACITY : ((bits & (kI | kF)) ? GG_MT_SHARING : GG_MT_COLD);
  }
};

// The slice of (tile, L1-D set) in cache `level` (0 L1-D, 1 L2) of the
// context's table (gg_mt_view, gg_internal.h).
__device__ __forceinline__ gg_mt_set gg_mt_set_of(const gg_mt_view& v, const gg_geom& g, uint32_t tile, uint32_t l1set,
                                                  int level)
{
  const uint32_t nc = v.on1 + v.on2;
  const bool on = level == 0 ? v.on1 != 0 : v.on2 != 0;
  const uint64_t ci = (level == 1 && v.on1) ? 1u : 0u;
  gg_mt_set m;
  m.s = on ? v.tab + (((((uint64_t)tile * nc + ci) << g.log_u1) + l1set) << v.log_spu) : nullptr;
  m.mask = (1u << v.log_spu) - 1;
  m.log_line = g.log_line;
  m.hshift = 64 - v.log_spu;
  m.log_u1 = g.log_u1;
  return m;
}

// The miss-type counts a lane gathers over a batch (three per cache, in
// registers; picked with compares, no register indexing).
struct gg_mt_counts {
  uint32_t c[2][GG_NUM_MISS_TYPES];
  __device__ __forceinline__ void clear()
  {
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int k = 0; k < GG_NUM_MISS_TYPES; ++k) c[l][k] = 0;
  }
  template <int L>
  __device__ __forceinline__ void add(uint32_t type)
  {
#pragma unroll
    for (int k = 0; k < GG_NUM_MISS_TYPES; ++k) c[L][k] += (type == (uint32_t)k) ? 1u : 0u;
  }
  __device__ __forceinline__ void flush(const gg_mt_view& v, uint32_t tile) const
  {
#pragma unroll
    for (int l = 0; l < 2; ++l)
#pragma unroll
      for (int k = 0; k < GG_NUM_MISS_TYPES; ++k)
        if (c[l][k]) atomicAdd(&v.cnt[((uint64_t)tile * 2 + l) * GG_NUM_MISS_TYPES + k], (unsigned long long)c[l][k]);
  }
};

// One access of the private replay, in the oracle's order (modep_access):
//   L1-D miss: L1.classify(a); no permission: L1 |= invalidated(a);
//   L2 miss: L2.classify(a); upgrade: L2 |= invalidated(a);
//   L2 install: L2.insert(a, l2ev, e2); L1-D holds the L2 victim: L1 |= invalidated(e2);
//   L1-D install: L1.insert(a, l1ev, e1).
// All arguments are byte addresses of lines; called for a lane whose access
// missed the L1-D.
__device__ __forceinline__ void gg_mt_access(const gg_mt_set& L1, const gg_mt_set& L2, gg_mt_counts& cnt, uint32_t& err,
                                             uint64_t a, bool inv1, bool miss2, bool upg, bool l2ev, uint64_t e2,
                                             bool invl1, bool l1ev, uint64_t e1)
{
  if (L1.on()) {
    cnt.add<0>(L1.classify(a, err));
    if (inv1) L1.or_bits(a, gg_mt_set::kI, err);
  }
  if (L2.on() && miss2) {
    cnt.add<1>(L2.classify(a, err));
    if (upg) L2.or_bits(a, gg_mt_set::kI, err);
    L2.insert(a, l2ev, e2, err);
  }
  if (L1.on()) {
    if (invl1) L1.or_bits(e2, gg_mt_set::kI, err);
    L1.insert(a, l1ev, e1, err);
  }
}
