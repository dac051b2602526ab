// gg_noc_many.h — what the ensemble entries (gg_noc_many.hip: gg_noc_route_batch_many,
// gg_noc_synthetic_run_many) ask of the units that own a
// context's NoC and synthetic-traffic state.  Host only.
#pragma once
#include <vector>

#include "gg_dev.h"
#include "gg_internal.h"

// A context's NoC state and batch scratch, grown for a batch of `cap` packets:
// what gg_noc_run / noc_hbh_stages would pass to their launches.  heap and pscr
// are the Ev and SK arrays of gg_noc.hip / gg_noc_stage.h.
struct gg_noc_view {
  gg::NocParams P;
  gg::HQueue* q; gg::HNode* nd;
  uint64_t* ctr;
  uint64_t *t, *zl, *ct;
  uint32_t *cur, *keys, *ids;
  void* heap;
  uint32_t *counts, *cursor;
  uint64_t* off;
  void* pscr; uint64_t pstride; uint32_t pk_max;
};
// The per-batch checks of gg_noc_run (its status, its words) and its scratch
// (noc_grow, pscr.reserve) for pk on ctx; nothing is launched.  num_packets > 0.
gg_status gg_noc_many_prepare(gg_ctx* ctx, const gg_packets* pk, const gg_packet_out* out, gg_noc_view* v);
// the stage-kernel form of the X / Y chains (NOC_FORM_*, gg_noc.hip), stage 1 or 2
int gg_noc_form(gg_ctx* ctx, int stage);
// the ensemble's instance table, kept by the set's first context (bytes of device memory)
gg_status gg_noc_many_table(gg_ctx* ctx, uint64_t bytes, void** dev);

// The launch constants and packet arrays of the synthetic-traffic generator
// (gg_noc_synth.hip: synth_prepare's result on the context's gg_synth_state).
struct gg_synth_plan {
  uint64_t* time;
  uint64_t* last_cycle;      // [tiles] or nullptr
  uint32_t* src;
  uint32_t* dst;
  uint32_t* len;
  uint32_t* aux;             // [0] stop flag; gg_noc_synthetic_run: [2 ..] the 2T-entry orbit table (uniform_random)
  uint64_t N, seed, thr, cycle_ps;
  uint32_t T, w, h, pattern, bits;
};
struct gg_synth_view {
  gg_synth_plan P;           // aux is left NULL: the ensemble keeps the stop words and the orbit in its own table
  uint64_t *arr, *zl, *ct;
};
// gg_noc_synthetic_run's checks of p (synth_prepare) and its arrays on ctx, grown; nothing is launched.
// orbit: uniform_random's destination table (2T entries, a function of the tile count alone), else empty
gg_status gg_synth_many_prepare(gg_ctx* ctx, const gg_traffic_params* p, gg_synth_view* v, std::vector<uint32_t>* orbit);
// the ensemble's table on the set's first context
gg_status gg_synth_many_table(gg_ctx* ctx, uint64_t bytes, void** dev);
