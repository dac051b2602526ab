// gg_stats.h — what the statistics trace (gg_stats.hip) sees of the coherent
// mode's state (gg_coherent.hip): the launch state the scan kernel reads.
#pragma once
#include "gg_coh_dev.h"

// The launch state of the context's coherent mode, allocated on first use as
// gg_coherent_begin does (nothing is reset or launched); *begun: a run has
// been begun on it.  The pointers live as long as the context.
gg_status gg_coh_launch_state(gg_ctx* ctx, const ggc::CP** P, const ggc::CS** S, bool* begun);

// The scan for an ensemble (gg_coherent_advance_many; k_stats_scan_many).  The
// driver keeps one record of gg_stats_many_bytes() per live instance beside
// its pair, fills it with the live list (an instance whose begun run has no
// trace: statistics = 0, the scan's workgroups leave at once) and launches one
// scan per slot, grid (tiles, live), while any live instance has a trace.
namespace ggc { struct ManyPair; }
uint32_t gg_stats_run_bits(const gg_ctx* ctx);       // GG_ST_* of the run begun last (0: no trace)
size_t   gg_stats_many_bytes();
void     gg_stats_many_fill(gg_ctx* ctx, const ggc::CS& S, void* rec);
void     gg_stats_many_slot(const ggc::ManyPair* pairs, const void* recs, uint32_t tiles, uint32_t live, size_t lds,
                            hipStream_t s, uint32_t L);

// The trace's part of a snapshot (gg_coherent_snapshot / _restore): the
// configuration of the run begun last, its header words and samples so far.
gg_status gg_stats_snapshot(gg_ctx* ctx, std::vector<uint64_t>& words);
bool      gg_stats_snapshot_ok(const gg_ctx* ctx, const uint64_t* w, uint64_t n);    // the words' shape (nothing changes)
gg_status gg_stats_restore_configure(gg_ctx* ctx, const uint64_t* w);              // before gg_coherent_begin
gg_status gg_stats_restore_upload(gg_ctx* ctx, const uint64_t* w, uint64_t n, hipStream_t s);   // after it
