// gg_snapshot.hip — a coherent run's snapshot on MI355X
// (gfx950): the kernels of its packed sections, then the host side of
// gg_coherent_snapshot / _restore.  The directory arrays are the bulk of a context's state
// and mostly never used; the sharer words of a never-used slot are not even
// initialised (gg_coh_dev.h, dfind).  So they leave the device as records
// {slot, entry, sharer words, Random word} of the slots in use, in slot order:
//   count    one workgroup per owned tile, 16-B entry loads, a wave sum
//   scan     exclusive over the tiles (one wave, DPP prefix)
//   pack     one workgroup per owned tile: ballot ranks inside a wave, the
//            waves' totals through LDS, so a tile's records keep slot order
// and come back by a scatter after the usual reset (unpack).  The miss-type
// address tables (~0 = empty) take the same three passes.
#include "gg_coh_host.h"
#include "gg_snapshot.h"
#include "gg_snapshot_win.h"
#include "gg_stats.h"

#include <algorithm>
#include <cstring>

namespace ggc {

constexpr uint32_t kSnapThreads = 256;

// slots [0, lim) of tile lt that a snapshot keeps
__device__ __forceinline__ uint32_t snap_limit(const PackSrc& s, uint32_t lt)
{
  return s.mode == PK_REP ? min(s.ts[lt].nrep, s.n) : s.n;
}
// PK_DIR: any field off its reset value {INV_ADDR, -1, UNCACHED, 0} (k_c_reset):
// an entry with a real address and no sharers holds its way, and a slot the
// engine opened had its sharer words zeroed then.  PK_REP: the live entries of
// the replaced list.  PK_TAB: an address-set slot that is not empty.
__device__ __forceinline__ bool snap_used(const PackSrc& s, uint32_t lt, uint32_t i, uint32_t lim)
{
  if (i >= lim) return false;
  if (s.mode == PK_REP) return true;
  const size_t g = (size_t)lt * s.n + i;
  if (s.mode == PK_TAB) return reinterpret_cast<const uint64_t*>(s.ent)[g] != ~0ull;
  const uint4 e = reinterpret_cast<const uint4*>(s.ent)[g];     // {addr lo, addr hi, owner, dstate | nsh << 16}
  return !(e.x == 0xFFFFFFFFu && e.y == 0xFFFFFFFFu && e.z == 0xFFFFFFFFu && e.w == 0u);
}

__global__ void __launch_bounds__(kSnapThreads) k_snap_count(PackSrc s, uint32_t* counts)
{
  __shared__ uint32_t tot;
  const uint32_t lt = blockIdx.x, tid = threadIdx.x;
  if (lt >= s.L) return;
  if (tid == 0) tot = 0;
  __syncthreads();
  const uint32_t lim = snap_limit(s, lt);
  uint32_t c = 0;
  for (uint32_t i = tid; i < lim; i += kSnapThreads) c += snap_used(s, lt, i, lim) ? 1u : 0u;
  c = wave_sum(c);
  if ((tid & 63) == 0 && c) atomicAdd(&tot, c);
  __syncthreads();
  if (tid == 0) counts[lt] = tot;
}

// base[lt] = records of the tiles before lt, base[L] = all (one wave)
__global__ void __launch_bounds__(64) k_snap_scan(const uint32_t* counts, uint32_t L, uint64_t* base)
{
  const uint32_t ln = threadIdx.x;
  uint64_t carry = 0;
  for (uint32_t c = 0; c < L; c += 64) {
    const uint32_t v = c + ln < L ? counts[c + ln] : 0u;
    const uint32_t ex = wave_excl_scan(v, ln);
    if (c + ln < L) base[c + ln] = carry + ex;
    carry += wave_sum(v);
  }
  if (ln == 0) base[L] = carry;
}

__global__ void __launch_bounds__(kSnapThreads) k_snap_pack(PackSrc s, const uint64_t* base, uint64_t cap, uint64_t* out)
{
  __shared__ uint32_t wt[kSnapThreads / 64];
  const uint32_t lt = blockIdx.x, tid = threadIdx.x, ln = tid & 63, wv = tid >> 6;
  if (lt >= s.L) return;
  const uint32_t lim = snap_limit(s, lt);
  const uint64_t b0 = base[lt];
  uint32_t run = 0;
  for (uint32_t c = 0; c < lim; c += kSnapThreads) {     // (uniform bounds: every thread takes every barrier)
    const uint32_t i = c + tid;
    const bool u = snap_used(s, lt, i, lim);
    const uint64_t m = __ballot(u);
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << ln) - 1ull));
    if (ln == 0) wt[wv] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t pre = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kSnapThreads / 64; ++w) { pre += w < wv ? wt[w] : 0u; all += wt[w]; }
    const uint64_t r = b0 + run + pre + rank;
    if (u && r < cap) {                                  // (cap = base[L] of the count pass: the state is at rest)
      const size_t g = (size_t)lt * s.n + i;
      uint64_t* o = out + r * s.rw;
      o[0] = g;
      if (s.mode == PK_TAB) o[1] = reinterpret_cast<const uint64_t*>(s.ent)[g];
      else {
        const uint4 e = reinterpret_cast<const uint4*>(s.ent)[g];
        o[1] = (uint64_t)e.x | ((uint64_t)e.y << 32);
        o[2] = (uint64_t)e.z | ((uint64_t)e.w << 32);
        for (uint32_t w = 0; w < s.W; ++w) o[3 + w] = s.sh[g * s.W + w];
        if (s.rng) o[3 + s.W] = s.rng[g];
      }
    }
    run += all;
    __syncthreads();
  }
}

// records back into their slots (after the run's reset); a slot index past
// the arrays is skipped (the host has checked them: defence in depth)
__global__ void __launch_bounds__(kSnapThreads) k_snap_unpack(PackSrc s, const uint64_t* recs, uint64_t n)
{
  const uint64_t r = (uint64_t)blockIdx.x * kSnapThreads + threadIdx.x;
  if (r >= n) return;
  const uint64_t* o = recs + r * s.rw;
  const uint64_t g = o[0];
  if (g >= (uint64_t)s.L * s.n) return;
  if (s.mode == PK_TAB) { reinterpret_cast<uint64_t*>(s.ent)[g] = o[1]; return; }
  reinterpret_cast<uint4*>(s.ent)[g] = make_uint4((uint32_t)o[1], (uint32_t)(o[1] >> 32), (uint32_t)o[2], (uint32_t)(o[2] >> 32));
  for (uint32_t w = 0; w < s.W; ++w) s.sh[g * s.W + w] = o[3 + w];
  if (s.rng) s.rng[g] = o[3 + s.W];
}

hipError_t snap_count(const PackSrc& s, uint32_t* counts, uint64_t* base, hipStream_t st)
{
  hipLaunchKernelGGL(k_snap_count, dim3(s.L), dim3(kSnapThreads), 0, st, s, counts);
  hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(64), 0, st, (const uint32_t*)counts, s.L, base);
  return hipGetLastError();
}
hipError_t snap_pack(const PackSrc& s, const uint64_t* base, uint64_t cap, uint64_t* out, hipStream_t st)
{
  hipLaunchKernelGGL(k_snap_pack, dim3(s.L), dim3(kSnapThreads), 0, st, s, base, cap, out);
  return hipGetLastError();
}
hipError_t snap_unpack(const PackSrc& s, const uint64_t* recs, uint64_t n, hipStream_t st)
{
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_snap_unpack, dim3((uint32_t)((n + kSnapThreads - 1) / kSnapThreads)), dim3(kSnapThreads), 0, st, s,
                     recs, n);
  return hipGetLastError();
}

}  // namespace ggc

using namespace ggc;
using namespace gg;

// ---------------------------------------------------------------------------
// snapshot / restore on the host (the container: gg_snapshot.h)
// ---------------------------------------------------------------------------
int snap_policy(const char* name)
{
  for (const char* k : {"dir", "dsh", "rep", "rsh", "drng", "rrng", "mtab", "l1_tag", "l2_tag"}) if (!std::strcmp(name, k)) return SN_PACKED;
  for (const char* k : {"pool0", "pool1", "bnd", "xl", "yl"}) if (!std::strcmp(name, k)) return SN_PREFIX;
  for (const char* k : {"gscr", "gbar"}) if (!std::strcmp(name, k)) return SN_NONE;
  return SN_DENSE;
}

static_assert(sizeof(CP) == 48 * 4 + 8 * 8 + sizeof(NocParams) && sizeof(NocParams) == 12 * 4 + 8,
              "the launch state is compared byte for byte: no padding");
namespace {
// the derived launch state a snapshot must meet again: CP and what coh_alloc
// derives beside it (env knobs included: they change P or these)
struct SnapLaunch { CP P; uint64_t wtx, wty, persist_lc, step_lds, walk_lds, diag; };
SnapLaunch snap_launch(const gg_coh_state* C)
{
  SnapLaunch l;
  std::memset(&l, 0, sizeof(l));
  l.P = C->P; l.wtx = C->wtx; l.wty = C->wty; l.persist_lc = C->persist_lc; l.step_lds = C->step_lds;
  l.walk_lds = C->walk_lds; l.diag = GG_COH_DIAG;
  return l;
}
// the packed sections: directory, replaced list, cache tags, miss-type tables
struct SnapPacked { const char* name; PackSrc src; };
std::vector<SnapPacked> snap_packed(const gg_coh_state* C)
{
  const CP& P = C->P; const CS& S = C->S;
  std::vector<SnapPacked> v;
  const uint32_t rw = 3 + P.W + (P.mosi ? 1u : 0u);
  v.push_back({"dir", PackSrc{(void*)S.dir, (uint64_t*)S.dsh, P.mosi ? (uint64_t*)S.drng : nullptr, nullptr, P.L, P.E, P.W, PK_DIR, rw}});
  v.push_back({"rep", PackSrc{(void*)S.rep, (uint64_t*)S.rsh, P.mosi ? (uint64_t*)S.rrng : nullptr, (const TileSt*)S.ts, P.L, P.R, P.W, PK_REP, rw}});
  v.push_back({"l1_tag", PackSrc{(void*)S.l1_tag, nullptr, nullptr, nullptr, P.L, P.s1 * P.a1, 0, PK_TAB, 2}});
  v.push_back({"l2_tag", PackSrc{(void*)S.l2_tag, nullptr, nullptr, nullptr, P.L, P.s2 * P.a2, 0, PK_TAB, 2}});
  if (S.mtab) v.push_back({"mtab", PackSrc{(void*)S.mtab, nullptr, nullptr, nullptr, P.L, 2u << P.mt_log, 0, PK_TAB, 2}});
  return v;
}
// the live counts of the prefix sections, from the count arrays (host copies)
struct SnapCounts { uint32_t npool[2], bnd; std::vector<uint32_t> nxl, nyl; };
uint64_t list_words(const std::vector<uint32_t>& n, uint32_t cap)
{
  uint64_t t = 0;
  for (uint32_t c : n) t += std::min(c, cap);
  return t;
}
gg_status snap_valid(gg_ctx* ctx, const char* what)
{
  GG_NOT_ATAC(ctx, what);
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun) return gg_fail(GG_ERR_INVALID, "%s: gg_coherent_begin or gg_coherent_restore first", what);
  if (gg_status st = coh_owns_all(ctx, GG_ERR_UNSUPPORTED, what)) return st;
  if (C->windowed)
    return gg_fail(GG_ERR_UNSUPPORTED, "%s: a run fed in windows (gg_coherent_begin_window) has no snapshot: "
                                       "the trace it continues on is not there yet", what);
  if (C->drv == gg_coh_state::DRV_HOST)
    return gg_fail(GG_ERR_INVALID, "%s: a run driven by gg_coherent_quantum / the round is not at the device loop's "
                                   "clean point (after begin, an advance or a restore)", what);
  return GG_OK;
}
// the same for a run fed in windows (gg_coherent_window_snapshot): the clean
// point is where a window may go in, or the end of the run
gg_status snap_valid_win(gg_ctx* ctx, const char* what)
{
  GG_NOT_ATAC(ctx, what);
  gg_coh_state* C = ctx->coh;
  if (!C || !C->begun)
    return gg_fail(GG_ERR_INVALID, "%s: gg_coherent_begin_window or gg_coherent_window_restore first", what);
  if (!C->windowed)
    return gg_fail(GG_ERR_INVALID, "%s: the run is not fed in windows: gg_coherent_snapshot takes its snapshot", what);
  hipSetDevice(ctx->device);
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  uint64_t done = 0;
  uint32_t err = 0;
  GG_HIP(hipMemcpy(&done, C->S.qs + QS_DONE, sizeof(done), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(&err, ctx->err_dev, sizeof(err), hipMemcpyDeviceToHost));
  if (err || (done & 3) == 2)
    return gg_fail(GG_ERR_INVALID, "%s: the run has failed%s: there is no state to continue from", what,
                   (err & GG_DERR_WINDOW) ? " (window exhausted)" : "");
  return GG_OK;
}
}  // namespace

// The records live at a quantum boundary and the lists that hold them, on the
// host.  quantum_end delivers the held records by atomics, so their pool
// slots and their order inside a list differ from run to run (every consumer
// orders by the canonical keys: the results do not).  A snapshot stores the
// canonical form — each list sorted by its records' bytes, the records packed
// from the pools' shared base in list order, as after k_c_round_commit's
// pool reset — so the same state gives the same bytes.
namespace {
struct SnapLive {
  std::vector<uint32_t> cnt4, inb0, inb1, arv0, arv1;
  std::vector<uint64_t> xl, yl;                        // the lists' live prefixes, run after run
  std::vector<gg_cmsg> pool0, pool1;
};
struct LiveRef { uint32_t list, idx; uint32_t* s32; uint64_t* s64; };
bool canon_pool(uint32_t base, uint32_t cap, uint32_t& npool, std::vector<gg_cmsg>& pool, std::vector<LiveRef>& refs)
{
  // every reference into the shared part, each record once: else the state is left as it is
  if (npool > cap || pool.size() != npool) return false;
  std::vector<bool> seen(npool, false);
  for (const LiveRef& r : refs) {
    if (r.idx < base || r.idx >= npool || seen[r.idx]) return false;
    seen[r.idx] = true;
  }
  if ((uint64_t)base + refs.size() > cap) return false;
  std::vector<gg_cmsg> out(pool.begin(), pool.begin() + std::min<size_t>(base, pool.size()));
  out.resize(base);                                    // (npool below the base: nothing was allocated yet)
  for (size_t a = 0; a < refs.size();) {
    size_t b = a;
    while (b < refs.size() && refs[b].list == refs[a].list) ++b;
    std::vector<gg_cmsg> recs;
    for (size_t i = a; i < b; ++i) recs.push_back(pool[refs[i].idx]);
    std::sort(recs.begin(), recs.end(), [](const gg_cmsg& x, const gg_cmsg& y) { return std::memcmp(&x, &y, sizeof(gg_cmsg)) < 0; });
    for (size_t i = a; i < b; ++i) {
      const uint32_t ni = (uint32_t)out.size();
      const gg_cmsg& m = recs[i - a];
      if (refs[i].s32) *refs[i].s32 = ni; else *refs[i].s64 = (uint64_t)ni | ((uint64_t)m.dst << 32);
      out.push_back(m);
    }
    a = b;
  }
  pool.swap(out);
  npool = (uint32_t)pool.size();
  return true;
}
}  // namespace

static gg_status snap_live(gg_coh_state* C, SnapCounts& n, SnapLive& v)
{
  const CP& P = C->P; const CS& S = C->S;
  const bool hbh = P.net == GG_NET_EMESH_HOP_BY_HOP;
  v.cnt4.resize((size_t)P.L * 4); v.inb0.resize((size_t)P.L * P.IC); v.arv1.resize(hbh ? (size_t)P.L * P.IC : 1);
  GG_HIP(hipMemcpy(v.cnt4.data(), S.cnt4, 4 * v.cnt4.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(v.inb0.data(), S.inb0, 4 * v.inb0.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(v.arv1.data(), S.arv1, 4 * v.arv1.size(), hipMemcpyDeviceToHost));
  v.inb1.resize(v.inb0.size()); v.arv0.resize(v.arv1.size());
  GG_HIP(hipMemcpy(v.inb1.data(), S.inb1, 4 * v.inb1.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(v.arv0.data(), S.arv0, 4 * v.arv0.size(), hipMemcpyDeviceToHost));
  // entries past a list's count are leftovers of earlier steps (slots handed
  // out by atomics): dead, and zero in a snapshot
  for (uint32_t lt = 0; lt < P.L; ++lt) {
    const uint32_t* c = &v.cnt4[(size_t)lt * 4];
    std::vector<uint32_t>* ls[4] = {&v.inb0, &v.inb1, &v.arv0, &v.arv1};
    for (int k = 0; k < 4; ++k) {
      if (k >= 2 && !hbh) continue;
      for (uint32_t j = std::min(c[k], P.IC); j < P.IC; ++j) (*ls[k])[(size_t)lt * P.IC + j] = 0;
    }
  }
  v.pool0.resize(std::min(n.npool[0], P.msg_cap)); v.pool1.resize(std::min(n.npool[1], P.msg_cap));
  if (!v.pool0.empty()) GG_HIP(hipMemcpy(v.pool0.data(), S.pool0, sizeof(gg_cmsg) * v.pool0.size(), hipMemcpyDeviceToHost));
  if (!v.pool1.empty()) GG_HIP(hipMemcpy(v.pool1.data(), S.pool1, sizeof(gg_cmsg) * v.pool1.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < 2; ++k) {
    const std::vector<uint32_t>& cnt = k ? n.nyl : n.nxl;
    std::vector<uint64_t>& o = k ? v.yl : v.xl;
    o.resize(list_words(cnt, P.seg_cap));
    size_t at = 0;
    for (size_t g = 0; g < cnt.size(); ++g) {
      const uint32_t c = std::min(cnt[g], P.seg_cap);
      if (c) GG_HIP(hipMemcpy(o.data() + at, (k ? S.yl : S.xl) + g * (size_t)P.seg_cap, 8ull * c, hipMemcpyDeviceToHost));
      at += c;
    }
  }
  // the references: inbox lists of the next quantum's step 0 into pool 1; its
  // SELF arrivals and run lists into pool 0 (import_one).  Lists of the other
  // parity hold nothing at a boundary; if they do, the state stays as it is.
  std::vector<LiveRef> r0, r1;
  uint32_t lid = 0;
  bool plain = true;
  for (uint32_t lt = 0; lt < P.L; ++lt, ++lid) {
    const uint32_t* c = &v.cnt4[(size_t)lt * 4];
    if (c[1] || c[2] || c[0] > P.IC || c[3] > P.IC || (!hbh && c[3])) { plain = false; break; }
    for (uint32_t j = 0; j < c[0]; ++j) { uint32_t* sl = &v.inb0[(size_t)lt * P.IC + j]; r1.push_back(LiveRef{lid, *sl, sl, nullptr}); }
  }
  for (uint32_t lt = 0; plain && hbh && lt < P.L; ++lt, ++lid)
    for (uint32_t j = 0; j < v.cnt4[(size_t)lt * 4 + 3]; ++j) { uint32_t* sl = &v.arv1[(size_t)lt * P.IC + j]; r0.push_back(LiveRef{lid, *sl, sl, nullptr}); }
  for (int k = 0; plain && k < 2; ++k) {
    const std::vector<uint32_t>& cnt = k ? n.nyl : n.nxl;
    std::vector<uint64_t>& o = k ? v.yl : v.xl;
    size_t at = 0;
    for (size_t g = 0; g < cnt.size(); ++g, ++lid)
      for (uint32_t j = 0; j < std::min(cnt[g], P.seg_cap); ++j, ++at) r0.push_back(LiveRef{lid, (uint32_t)o[at], nullptr, &o[at]});
  }
  if (!plain) return GG_OK;
  // (both pools or neither: copies, committed together)
  SnapLive w = v;
  auto rebase = [&](std::vector<LiveRef>& rs) {
    for (LiveRef& r : rs) {
      if (r.s32) r.s32 = (r.s32 >= v.inb0.data() && r.s32 < v.inb0.data() + v.inb0.size()) ? w.inb0.data() + (r.s32 - v.inb0.data())
                                                                                          : w.arv1.data() + (r.s32 - v.arv1.data());
      else r.s64 = (r.s64 >= v.xl.data() && r.s64 < v.xl.data() + v.xl.size()) ? w.xl.data() + (r.s64 - v.xl.data())
                                                                               : w.yl.data() + (r.s64 - v.yl.data());
    }
  };
  rebase(r0); rebase(r1);
  uint32_t np0 = (uint32_t)w.pool0.size(), np1 = (uint32_t)w.pool1.size();
  const uint32_t base = P.L * kChunk;
  if (np0 != n.npool[0] || np1 != n.npool[1]) return GG_OK;
  if (!canon_pool(base, P.msg_cap, np0, w.pool0, r0) || !canon_pool(base, P.msg_cap, np1, w.pool1, r1)) return GG_OK;
  v = std::move(w);
  n.npool[0] = np0; n.npool[1] = np1;
  return GG_OK;
}

// host_buf == nullptr: the size only
// win: of a run fed in windows.  The tiles' positions leave as counts of
// consumed records (S.ts from the gather kernel's canonical copy, the offsets
// section as the prefix sums of the counts), the record each tile stands on
// in the win section: no byte depends on where the windows were cut.
static gg_status coh_snapshot(gg_ctx* ctx, uint8_t* host_buf, uint64_t cap, uint64_t* bytes, bool win)
{
  gg_coh_state* C = ctx->coh;
  const CP& P = C->P; const CS& S = C->S;
  hipSetDevice(ctx->device);
  hipStream_t s = ctx->last_stream;
  GG_HIP(hipStreamSynchronize(s));
  if (gg_status e = gg_coh_check(ctx)) return e;
  SnapCounts n;
  n.nxl.resize(std::max(P.nsx, 1u)); n.nyl.resize(std::max(P.nsy, 1u));
  GG_HIP(hipMemcpy(n.npool, S.npool, sizeof(n.npool), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(&n.bnd, S.bnd_cnt, sizeof(uint32_t), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(n.nxl.data(), S.nxl, sizeof(uint32_t) * n.nxl.size(), hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(n.nyl.data(), S.nyl, sizeof(uint32_t) * n.nyl.size(), hipMemcpyDeviceToHost));
  SnapLive live;
  if (gg_status e = snap_live(C, n, live)) return e;
  std::vector<uint64_t> stw;
  if (gg_status e = gg_stats_snapshot(ctx, stw)) return e;
  std::vector<SnapPacked> pk = snap_packed(C);
  std::vector<std::vector<uint64_t>> base(pk.size(), std::vector<uint64_t>((size_t)P.L + 1));
  for (size_t i = 0; i < pk.size(); ++i) {
    GG_HIP(snap_count(pk[i].src, C->pk_counts, C->pk_base, s));
    GG_HIP(hipMemcpyAsync(base[i].data(), C->pk_base, sizeof(uint64_t) * (P.L + 1), hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
  }
  const SnapLaunch sl = snap_launch(C);
  const uint64_t nqueues = (uint64_t)P.T * 6 + 1;
  ggsnap::Layout lay;
  lay.add("cfg", ggsnap::SK_DENSE, 0, sizeof(gg_config), 0);
  lay.add("launch", ggsnap::SK_DENSE, 0, sizeof(SnapLaunch), 0);
  lay.add("offsets", ggsnap::SK_DENSE, 0, sizeof(uint64_t) * (P.T + 1), 0);
  lay.add("stats", ggsnap::SK_DENSE, 0, sizeof(uint64_t) * stw.size(), 0);
  lay.add("err", ggsnap::SK_DENSE, 0, 2 * sizeof(uint32_t), 0);
  lay.add("noc_ctr", ggsnap::SK_DENSE, 0, sizeof(uint64_t) * P.T * GG_NUM_NET_COUNTERS, 0);
  lay.add("noc_q", ggsnap::SK_DENSE, 0, sizeof(HQueue) * nqueues, 0);
  lay.add("noc_nd", ggsnap::SK_DENSE, 0, sizeof(HNode) * nqueues * P.np.max_size, 0);
  const size_t first_arr = lay.sec.size();
  for (const gg_coh_state::Arr& a : C->arrs) {
    const int pol = snap_policy(a.name);
    if (pol == SN_DENSE) lay.add(a.name, ggsnap::SK_DENSE, 0, a.bytes, 0);
    else if (pol == SN_PREFIX) {
      uint64_t b = 0;
      if (!std::strcmp(a.name, "pool0")) b = sizeof(gg_cmsg) * std::min(n.npool[0], P.msg_cap);
      else if (!std::strcmp(a.name, "pool1")) b = sizeof(gg_cmsg) * std::min(n.npool[1], P.msg_cap);
      else if (!std::strcmp(a.name, "bnd")) b = sizeof(gg_cmsg) * std::min(n.bnd, P.msg_cap);
      else if (!std::strcmp(a.name, "xl")) b = 8 * list_words(n.nxl, P.seg_cap);
      else b = 8 * list_words(n.nyl, P.seg_cap);
      lay.add(a.name, ggsnap::SK_DENSE, 0, b, 0);
    }
  }
  const size_t first_pk = lay.sec.size();
  for (size_t i = 0; i < pk.size(); ++i)
    lay.add(pk[i].name, ggsnap::SK_PACKED, pk[i].src.rw * 8, base[i][P.L] * pk[i].src.rw * 8, base[i][P.L]);
  const size_t win_sec = lay.sec.size();
  if (win) lay.add(ggsnap::kWinSection, ggsnap::SK_DENSE, 0, sizeof(ggsnap::WinRec) * P.T, 0);
  const uint64_t total = lay.finish();
  *bytes = total;
  if (!host_buf) return GG_OK;
  if (cap < total) return gg_fail(GG_ERR_RANGE, "snapshot needs %llu bytes, the buffer holds %llu",
                                  (unsigned long long)total, (unsigned long long)cap);
  // (the padding between sections is part of the checksummed payload: zero)
  for (size_t i = 0; i < lay.sec.size(); ++i) {
    const uint64_t e = lay.sec[i].off + lay.sec[i].bytes, nx = i + 1 < lay.sec.size() ? lay.sec[i + 1].off : total;
    if (nx > e) std::memset(host_buf + e, 0, nx - e);
  }
  auto at = [&](size_t i) { return host_buf + lay.sec[i].off; };
  std::vector<TileSt> wts;
  std::vector<uint64_t> wrec, offs(C->offs_host);
  if (win) {
    if (gg_status e = coh_window_gather(ctx, wts, wrec)) return e;
    offs.assign((size_t)P.T + 1, 0);
    for (uint32_t t = 0; t < P.T; ++t) offs[t + 1] = offs[t] + wrec[(size_t)4 * t];
    std::memcpy(at(win_sec), wrec.data(), lay.sec[win_sec].bytes);
  }
  if (offs.size() != (size_t)P.T + 1) return gg_fail(GG_ERR_STATE, "snapshot: the bound trace's offsets");
  std::memcpy(at(0), &ctx->cfg, sizeof(gg_config));
  std::memcpy(at(1), &sl, sizeof(sl));
  std::memcpy(at(2), offs.data(), lay.sec[2].bytes);
  std::memcpy(at(3), stw.data(), lay.sec[3].bytes);
  GG_HIP(hipMemcpy(at(4), ctx->err_dev, lay.sec[4].bytes, hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(at(5), S.ctr, lay.sec[5].bytes, hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(at(6), S.nq, lay.sec[6].bytes, hipMemcpyDeviceToHost));
  GG_HIP(hipMemcpy(at(7), S.nnd, lay.sec[7].bytes, hipMemcpyDeviceToHost));
  size_t si = first_arr;
  for (const gg_coh_state::Arr& a : C->arrs) {
    const int pol = snap_policy(a.name);
    if (pol != SN_DENSE && pol != SN_PREFIX) continue;
    const ggsnap::Section& sec = lay.sec[si];
    // the live records and their lists come from the host copies (snap_live)
    const void* host = nullptr;
    uint64_t hb = 0;
    auto from = [&](const char* nm, const void* p, uint64_t b) { if (!std::strcmp(a.name, nm)) { host = p; hb = b; } };
    from("npool", n.npool, sizeof(n.npool));
    from("inb0", live.inb0.data(), 4 * live.inb0.size()); from("arv1", live.arv1.data(), 4 * live.arv1.size());
    from("inb1", live.inb1.data(), 4 * live.inb1.size()); from("arv0", live.arv0.data(), 4 * live.arv0.size());
    from("xl", live.xl.data(), 8 * live.xl.size()); from("yl", live.yl.data(), 8 * live.yl.size());
    from("pool0", live.pool0.data(), sizeof(gg_cmsg) * live.pool0.size());
    from("pool1", live.pool1.data(), sizeof(gg_cmsg) * live.pool1.size());
    if (win) from("ts", wts.data(), sizeof(TileSt) * wts.size());
    if (host) {
      if (hb != sec.bytes) return gg_fail(GG_ERR_STATE, "snapshot: section %s changed size while it was taken", a.name);
      if (hb) std::memcpy(at(si), host, hb);
    }
    else if (sec.bytes) GG_HIP(hipMemcpy(at(si), a.p, sec.bytes, hipMemcpyDeviceToHost));
    // the launch index is not state: a resume restarts it at 0 (QS_START = 0,
    // S.live[] zeroed), and the launch forms count differently — the ensemble
    // ends a quantum in a step launch, the single hop-by-hop run in a walker
    // launch.  Both words leave as a resume sets them, so the same state gives
    // the same bytes whoever drove the run.
    if (!std::strcmp(a.name, "qs")) std::memset(at(si) + sizeof(uint64_t) * QS_START, 0, sizeof(uint64_t));
    if (!std::strcmp(a.name, "ring")) std::memset(at(si) + sizeof(uint32_t) * 7, 0, sizeof(uint32_t) * 4);
    // a pause for the next windows (kQsWindow) is a pause: whether the run
    // stopped for them or for the caller's stop depends on the cuts
    if (win && !std::strcmp(a.name, "qs")) {
      uint64_t d;
      std::memcpy(&d, at(si) + sizeof(uint64_t) * QS_DONE, sizeof(d));
      if (d == kQsWindow) { d = kQsPaused; std::memcpy(at(si) + sizeof(uint64_t) * QS_DONE, &d, sizeof(d)); }
    }
    ++si;
  }
  for (size_t i = 0; i < pk.size(); ++i) {
    const ggsnap::Section& sec = lay.sec[first_pk + i];
    if (!sec.bytes) continue;
    if (gg_status e = C->pk_stage.reserve(sec.bytes)) return e;
    GG_HIP(hipMemcpyAsync(C->pk_base, base[i].data(), sizeof(uint64_t) * (P.L + 1), hipMemcpyHostToDevice, s));
    GG_HIP(snap_pack(pk[i].src, C->pk_base, sec.records, reinterpret_cast<uint64_t*>(C->pk_stage.get()), s));
    GG_HIP(hipMemcpyAsync(at(first_pk + i), C->pk_stage, sec.bytes, hipMemcpyDeviceToHost, s));
    GG_HIP(hipStreamSynchronize(s));
  }
  lay.write(host_buf, total);
  return GG_OK;
}

gg_status gg_coherent_snapshot_size(gg_ctx* ctx, uint64_t* bytes)
{
  if (!ctx || !bytes) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = snap_valid(ctx, "gg_coherent_snapshot_size")) return st;
  return coh_snapshot(ctx, nullptr, 0, bytes, false);
}

gg_status gg_coherent_snapshot(gg_ctx* ctx, void* host_buf, uint64_t cap, uint64_t* bytes)
{
  if (!ctx || !bytes || !host_buf) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = snap_valid(ctx, "gg_coherent_snapshot")) return st;
  return coh_snapshot(ctx, (uint8_t*)host_buf, cap, bytes, false);
}

gg_status gg_coherent_window_snapshot_size(gg_ctx* ctx, uint64_t* bytes)
{
  if (!ctx || !bytes) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = snap_valid_win(ctx, "gg_coherent_window_snapshot_size")) return st;
  return coh_snapshot(ctx, nullptr, 0, bytes, true);
}

gg_status gg_coherent_window_snapshot(gg_ctx* ctx, void* host_buf, uint64_t cap, uint64_t* bytes)
{
  if (!ctx || !bytes || !host_buf) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (gg_status st = snap_valid_win(ctx, "gg_coherent_window_snapshot")) return st;
  return coh_snapshot(ctx, (uint8_t*)host_buf, cap, bytes, true);
}

gg_status gg_window_snapshot_state(const void* host_buf, uint64_t bytes, uint32_t num_tiles, uint64_t* consumed,
                                   uint8_t* finished)
{
  if (const char* why = ggsnap::win_read(host_buf, bytes, num_tiles, consumed, finished))
    return gg_fail(GG_ERR_INVALID, "gg_window_snapshot_state: %s", why);
  return GG_OK;
}

// windowed: gg_coherent_window_restore — tr is the tiles' first windows (tile
// t's range begins at record consumed[t] of its trace), final_tiles as in
// gg_coherent_begin_window; otherwise gg_coherent_restore over the whole trace
static gg_status coh_restore(gg_ctx* ctx, const char* const what, bool windowed, const gg_trace* tr, uint64_t* access_out_dev,
                             const uint8_t* final_tiles, const void* host_buf, uint64_t bytes, void* stream)
{
  GG_NOT_ATAC(ctx, what);
  if (!ctx || !tr || !tr->tile_offsets || !host_buf) return gg_fail(GG_ERR_INVALID, "%s: NULL argument", what);
  if (gg_status st = coh_owns_all(ctx, GG_ERR_UNSUPPORTED, what)) return st;
  hipSetDevice(ctx->device);
  if (gg_status st = coh_alloc(ctx)) return st;
  gg_coh_state* C = ctx->coh;
  const CP& P = C->P;
  if (windowed && P.lat_l1d == 0)
    return gg_fail(GG_ERR_UNSUPPORTED, "%s: with zero L1-D data cycles a record can cost no time, so no window "
                                       "bounds what a tile consumes in a quantum", what);
  // ---- everything is checked before anything is changed ----
  ggsnap::View v;
  if (const char* why = ggsnap::parse(host_buf, bytes, &v)) return gg_fail(GG_ERR_INVALID, "%s: %s", what, why);
  auto bad = [what](const char* why) { return gg_fail(GG_ERR_INVALID, "%s: %s", what, why); };
  const uint8_t* wrecs = nullptr;
  if (!windowed && v.find(ggsnap::kWinSection))
    return bad("the snapshot is of a run fed in windows: gg_coherent_window_restore takes it");
  if (windowed)
    if (const char* why = ggsnap::win_section(v, P.T, &wrecs)) return bad(why);
  auto dense = [&](const char* name, uint64_t want) -> const ggsnap::Section* {
    const ggsnap::Section* x = v.find(name);
    return x && x->kind == ggsnap::SK_DENSE && x->bytes == want ? x : nullptr;
  };
  const ggsnap::Section* x;
  if (!(x = dense("cfg", sizeof(gg_config))) || std::memcmp(v.data(*x), &ctx->cfg, sizeof(gg_config)))
    return bad("the snapshot was taken under a different gg_config");
  const SnapLaunch sl = snap_launch(C);
  if (!(x = dense("launch", sizeof(SnapLaunch))) || std::memcmp(v.data(*x), &sl, sizeof(sl)))
    return bad("the snapshot was taken under a different derived launch state (environment knobs, build)");
  if (!(x = dense("offsets", sizeof(uint64_t) * (P.T + 1))) ||
      (!windowed && std::memcmp(v.data(*x), tr->tile_offsets, x->bytes)))
    return bad("the trace's tile_offsets are not the snapshot's");
  const ggsnap::Section* xst = v.find("stats");
  if (!xst || xst->kind != ggsnap::SK_DENSE || (xst->bytes & 7)) return bad("statistics-trace section");
  std::vector<uint64_t> stw(xst->bytes / 8);
  std::memcpy(stw.data(), v.data(*xst), xst->bytes);
  if (!gg_stats_snapshot_ok(ctx, stw.data(), stw.size())) return bad("statistics-trace section does not fit the context");
  const uint64_t nqueues = (uint64_t)P.T * 6 + 1;
  const ggsnap::Section* xerr = dense("err", 2 * sizeof(uint32_t));
  const ggsnap::Section* xctr = dense("noc_ctr", sizeof(uint64_t) * P.T * GG_NUM_NET_COUNTERS);
  const ggsnap::Section* xq = dense("noc_q", sizeof(HQueue) * nqueues);
  const ggsnap::Section* xnd = dense("noc_nd", sizeof(HNode) * nqueues * P.np.max_size);
  if (!xerr || !xctr || !xq || !xnd) return bad("a NoC or error-word section is missing or its size disagrees with the context");
  for (const gg_coh_state::Arr& a : C->arrs)
    if (snap_policy(a.name) == SN_DENSE && !dense(a.name, a.bytes))
      return gg_fail(GG_ERR_INVALID, "%s: section %s is missing or its size disagrees with the context", what, a.name);
  // the prefix sections against the counts the snapshot itself carries
  SnapCounts n;
  n.nxl.resize(std::max(P.nsx, 1u)); n.nyl.resize(std::max(P.nsy, 1u));
  std::memcpy(n.npool, v.data(*v.find("npool")), sizeof(n.npool));
  std::memcpy(&n.bnd, v.data(*v.find("bnd_cnt")), sizeof(uint32_t));
  std::memcpy(n.nxl.data(), v.data(*v.find("nxl")), sizeof(uint32_t) * n.nxl.size());
  std::memcpy(n.nyl.data(), v.data(*v.find("nyl")), sizeof(uint32_t) * n.nyl.size());
  if (!dense("pool0", sizeof(gg_cmsg) * std::min(n.npool[0], P.msg_cap)) ||
      !dense("pool1", sizeof(gg_cmsg) * std::min(n.npool[1], P.msg_cap)) ||
      !dense("bnd", sizeof(gg_cmsg) * std::min(n.bnd, P.msg_cap)) ||
      !dense("xl", 8 * list_words(n.nxl, P.seg_cap)) || !dense("yl", 8 * list_words(n.nyl, P.seg_cap)))
    return bad("a record pool or list section disagrees with its count");
  std::vector<SnapPacked> pk = snap_packed(C);
  for (const SnapPacked& p : pk) {
    x = v.find(p.name);
    const uint64_t slots = (uint64_t)p.src.L * p.src.n;
    if (!x || x->kind != ggsnap::SK_PACKED || x->rec_bytes != p.src.rw * 8 || x->records > slots)
      return gg_fail(GG_ERR_INVALID, "%s: packed section %s is missing or does not fit the context", what, p.name);
    const uint8_t* r = v.data(*x);
    uint64_t prev = 0;
    for (uint64_t i = 0; i < x->records; ++i, r += x->rec_bytes) {   // slot indices: inside the arrays, ascending
      uint64_t g;
      std::memcpy(&g, r, 8);
      if (g >= slots || (i && g <= prev))
        return gg_fail(GG_ERR_INVALID, "%s: packed section %s, record %llu: slot index", what, p.name, (unsigned long long)i);
      prev = g;
    }
  }
  if (windowed) {
    // the windows against the records the tiles stood on (a device pass that reads no run state)
    if (gg_status st = coh_trace_check(tr, P.T, what)) return st;
    if (gg_status st = coh_window_restore_check(ctx, what, tr, final_tiles, wrecs, (hipStream_t)stream)) return st;
  }
  // ---- the usual reset, then the state ----
  if (gg_status st = gg_stats_restore_configure(ctx, stw.data())) return st;
  if (gg_status st = gg_coherent_begin(ctx, tr, access_out_dev, stream)) return st;
  // (from here a failure of a windowed restore leaves no begun run, as in gg_coherent_begin_window)
  struct Unbegin { gg_coh_state* C; bool on; ~Unbegin() { if (on) { C->begun = false; C->windowed = false; C->S.win = nullptr; } } }
      unbegin{C, windowed};
  hipStream_t s = ctx->last_stream;
  const CS& S = C->S;
  if (gg_status st = gg_stats_restore_upload(ctx, stw.data(), stw.size(), s)) return st;
  GG_HIP(hipMemcpy(ctx->err_dev, v.data(*xerr), xerr->bytes, hipMemcpyHostToDevice));
  GG_HIP(hipMemcpy(S.ctr, v.data(*xctr), xctr->bytes, hipMemcpyHostToDevice));
  GG_HIP(hipMemcpy(S.nq, v.data(*xq), xq->bytes, hipMemcpyHostToDevice));
  GG_HIP(hipMemcpy(S.nnd, v.data(*xnd), xnd->bytes, hipMemcpyHostToDevice));
  for (const gg_coh_state::Arr& a : C->arrs) {
    const int pol = snap_policy(a.name);
    if (pol != SN_DENSE && pol != SN_PREFIX) continue;
    x = v.find(a.name);
    const bool lists = !std::strcmp(a.name, "xl") || !std::strcmp(a.name, "yl");
    if (!lists) { if (x->bytes) GG_HIP(hipMemcpy(a.p, v.data(*x), x->bytes, hipMemcpyHostToDevice)); }
    else {
      const std::vector<uint32_t>& cnt = a.name[0] == 'x' ? n.nxl : n.nyl;
      const uint8_t* o = v.data(*x);
      for (size_t g = 0; g < cnt.size(); ++g) {
        const uint64_t b = 8ull * std::min(cnt[g], P.seg_cap);
        if (b) GG_HIP(hipMemcpy((uint8_t*)a.p + g * 8ull * P.seg_cap, o, b, hipMemcpyHostToDevice));
        o += b;
      }
    }
  }
  for (const SnapPacked& p : pk) {
    x = v.find(p.name);
    if (!x->bytes) continue;
    if (gg_status st = C->pk_stage.reserve(x->bytes)) return st;
    GG_HIP(hipMemcpyAsync(C->pk_stage, v.data(*x), x->bytes, hipMemcpyHostToDevice, s));
    GG_HIP(snap_unpack(p.src, reinterpret_cast<const uint64_t*>(C->pk_stage.get()), x->records, s));
    GG_HIP(hipStreamSynchronize(s));
  }
  GG_HIP(hipStreamSynchronize(s));
  C->drv = gg_coh_state::DRV_DEVICE;                  // a snapshot is of the device loop's state
  if (windowed) {
    if (gg_status st = coh_window_restore_install(ctx, tr, s)) return st;
    unbegin.on = false;
  }
  return GG_OK;
}

gg_status gg_coherent_restore(gg_ctx* ctx, const gg_trace* tr, uint64_t* access_out_dev, const void* host_buf,
                              uint64_t bytes, void* stream)
{
  return coh_restore(ctx, "gg_coherent_restore", false, tr, access_out_dev, nullptr, host_buf, bytes, stream);
}

gg_status gg_coherent_window_restore(gg_ctx* ctx, const gg_trace* win, uint64_t* access_out_dev, const uint8_t* final_tiles,
                                     const void* host_buf, uint64_t bytes, void* stream)
{
  return coh_restore(ctx, "gg_coherent_window_restore", true, win, access_out_dev, final_tiles, host_buf, bytes, stream);
}
