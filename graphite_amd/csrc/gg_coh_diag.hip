// gg_coh_diag.hip — what a diagnostics build (GG_COH_DIAG) writes out after
// the device loop: the raw launch traces (GG_COH_TRACE_OUT) and the profile
// (GG_COH_PROFILE; the words: gg_coh_prof.h).  Host code only.
#include "gg_coh_host.h"

#include <algorithm>
#include <string>

using namespace ggc;

gg_status coh_diag_dump(gg_ctx* ctx)
{
  gg_coh_state* C = ctx->coh;
  const CP& P = C->P;
  if (C->S.trs && getenv("GG_COH_TRACE_OUT")) {
    // raw dumps for tools/coh_trace.py: steps [n][L][16], walkers [n][2][wb][8] (u64)
    const std::string pre = getenv("GG_COH_TRACE_OUT");
    const size_t ns = (size_t)C->S.tr_n * P.L * kTrStep, nw = (size_t)C->S.tr_n * 2 * C->S.tr_wb * 8;
    std::vector<unsigned long long> h(std::max(ns, nw));
    for (int k = 0; k < 2; ++k) {
      const size_t cnt = k ? nw : ns;
      GG_HIP(hipMemcpy(h.data(), k ? C->S.trw : C->S.trs, 8 * cnt, hipMemcpyDeviceToHost));
      if (FILE* f = fopen((pre + (k ? ".walk" : ".step")).c_str(), "wb")) { fwrite(h.data(), 8, cnt, f); fclose(f); }
    }
    if (C->S.tre) {
      const size_t ne = (size_t)C->S.tre_n * 2 * C->S.tr_wb * (kTrEvMax * 4 + 4);
      std::vector<unsigned long long> he(ne);
      GG_HIP(hipMemcpy(he.data(), C->S.tre, 8 * ne, hipMemcpyDeviceToHost));
      if (FILE* f = fopen((pre + ".ev").c_str(), "wb")) { fwrite(he.data(), 8, ne, f); fclose(f); }
    }
    if (FILE* f = fopen((pre + ".meta").c_str(), "w")) {
      fprintf(f, "{\"launches\": %u, \"tiles\": %u, \"walk_blocks\": %u, \"nsx\": %u, \"nsy\": %u, \"wtx\": %u, \"wty\": %u, "
              "\"ev_first\": %u, \"ev_launches\": %u, \"ev_max\": %u}\n",
              C->S.tr_n, P.L, C->S.tr_wb, P.nsx, P.nsy, C->wtx, C->wty, kTrEv0, C->S.tre_n, kTrEvMax);
      fclose(f);
    }
  }
  if (!C->S.prof) return GG_OK;
  std::vector<unsigned long long> h(PF_WORDS);
  GG_HIP(hipMemcpy(h.data(), C->S.prof, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
  // the per-launch maxima, summed over their rings
  unsigned long long crit = 0, wx = 0, wy = 0, mt = 0, mx = 0, my = 0;
  for (int i = 0; i < PF_RING; ++i) {
    crit += h[PF_R_STEP + i]; wx += h[PF_R_WALK + 2 * i]; wy += h[PF_R_WALK + 2 * i + 1];
    mt += h[PF_R_STEP_REQ + i]; mx += h[PF_R_WALK_REQ + 2 * i]; my += h[PF_R_WALK_REQ + 2 * i + 1];
  }
  const unsigned long long* sw = &h[PF_SWEEP];
  fprintf(stderr, "[gg_coh] step cycles over tiles: self %llu inbox+handlers %llu (order %llu) trace %llu publish %llu "
          "writeback %llu | slowest tile per launch %llu\n"
          "[gg_coh] walkers: %llu launches, staging %llu events %llu loop %llu handoff %llu, max events X %llu Y %llu | "
          "slowest walker per launch X %llu Y %llu | sweep: batch %llu queue load %llu requests %llu store %llu (s_memtime cycles); requests fast %llu M/G/1 %llu search %llu\n",
          h[PF_STEP_SELF], h[PF_STEP_INBOX], h[PF_STEP_ORDER], h[PF_STEP_TRACE], h[PF_STEP_PUBLISH], h[PF_STEP_WRITEBACK], crit,
          h[PF_WALK_LAUNCHES], h[PF_WALK_STAGE], h[PF_WALK_EVENTS], h[PF_WALK_LOOP], h[PF_WALK_HANDOFF], h[PF_WALK_MAXEV],
          h[PF_WALK_MAXEV + 1], wx, wy, sw[0], sw[1], sw[2], sw[3], sw[4], sw[5], sw[6]);
  const unsigned long long* sp = &h[PF_SELF_PHASE];
  fprintf(stderr, "[gg_coh] tiles with SELF arrivals: %llu; cycles prologue %llu, narv %llu, gather %llu, order %llu, queue load %llu, "
          "requests + store %llu | tiles without: %llu, prologue %llu\n", h[PF_SELF_TILES], sp[0], sp[1], sp[2], sp[3], sp[4], sp[5],
          h[PF_NOSELF_TILES], h[PF_NOSELF_PROLOGUE]);
  fprintf(stderr, "[gg_coh] per-launch max requests summed: tile (self+sent) %llu walker X %llu Y %llu\n", mt, mx, my);
  fprintf(stderr, "[gg_coh] walkers: most packets in one run X %llu Y %llu; pipelined runs past 64 packets (a lane's second "
          "candidate; past 128 wave 0 sweeps) %llu\n", h[PF_WALK_MAXPK], h[PF_WALK_MAXPK + 1], h[PF_WALK_PAST64]);
  const unsigned long long serves = h[PF_WALK_EVENTS];
  fprintf(stderr, "[gg_coh] walkers, armed waits: arms %llu hits %llu (%.1f %% of %llu serves) misses %llu; "
          "same-bound continues %llu\n", h[PF_ARM], h[PF_ARM_HIT], serves ? 100.0 * (double)h[PF_ARM_HIT] / (double)serves : 0.0,
          serves, h[PF_ARM_MISS], h[PF_ARM_CONT]);
  unsigned long long sn = 0, sa = 0, ss = 0, c1 = 0, c2 = 0, c3 = 0, ct = 0, nl = 0;
  for (int i = 0; i < PF_SHAPES; ++i) {
    const unsigned long long* b = &h[PF_R_SHAPE + 4 * i];
    if (!b[0]) continue;
    ++nl; ct += b[0] >> 24;
    sn += (b[0] >> 16) & 255; sa += (b[0] >> 8) & 255; ss += b[0] & 255;
    c1 += (b[1] & 0xFFFFFF) << 8; c2 += (b[2] & 0xFFFFFF) << 8; c3 += (b[3] & 0xFFFFFF) << 8;
  }
  fprintf(stderr, "[gg_coh] slowest tile per launch (%llu launches, last 16384 indices): cycles %llu; inbox msgs %llu, SELF arrivals %llu, "
          "sent %llu; cycles self-phase %llu inbox+handlers %llu trace %llu\n", nl, ct, sn, sa, ss, c1, c2, c3);
  const char* kn[3] = {"SELF", "injection", "walker"};
  for (int k = 0; k < 3; ++k) {
    const unsigned long long* b = &h[PF_BATCH + PF_BATCH_KIND * k];
    fprintf(stderr, "[gg_coh] %s batches, requests by size 1|2-3|4-7|8-15|16-31|32-63|64+: %llu %llu %llu %llu %llu %llu %llu; tail requests %llu\n",
            kn[k], b[0], b[1], b[2], b[3], b[4], b[5], b[6], h[PF_BATCH_TAIL + k]);
  }
  fprintf(stderr, "[gg_coh] trace: hit runs %llu cycles for %llu records (%llu calls, look-up part %llu; %llu row updates: "
          "loop %llu stores %llu); other accesses %llu cycles for %llu\n",
          h[PF_HR_CYCLES], h[PF_HR_RECORDS], h[PF_HR_CALLS], h[PF_HR_T_LOOKUP] - h[PF_HR_T_START], h[PF_HR_ROWS],
          h[PF_HR_T_LOOP] - h[PF_HR_T_LOOKUP], h[PF_HR_T_STORE] - h[PF_HR_T_LOOP], h[PF_ACC_CYCLES], h[PF_ACC_COUNT]);
  return GG_OK;
}
