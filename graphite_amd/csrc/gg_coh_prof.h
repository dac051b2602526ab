// gg_coh_prof.h — the words of CS::prof (GG_COH_PROFILE=1 in a diagnostics
// build): shader-clock cycles and counts the step and walker bodies add up
// (gg_coh_dev.h) and coh_diag_dump prints (gg_coh_diag.hip).  Included by
// gg_coh_dev.h beside CS; in a file of its own because fail() records the line
// of gg_coh_dev.h it was called from, so that file's line numbers are part of
// the compiled kernels.
#pragma once

enum {
  // a step, summed over tiles: cycles of its phases
  PF_STEP_SELF = 0, PF_STEP_INBOX, PF_STEP_TRACE, PF_STEP_PUBLISH, PF_STEP_WRITEBACK,
  PF_STEP_ORDER = 9,                   // of PF_STEP_INBOX: ordering the inbox
  // a walker launch, summed over runs: cycles of staging, event loop and hand-off; events; launches
  PF_WALK_STAGE = 16, PF_WALK_LOOP, PF_WALK_HANDOFF, PF_WALK_EVENTS, PF_WALK_LAUNCHES = 22,
  PF_WALK_MAXEV = 24,                  // [stage] the most events of one run
  PF_SWEEP = 26,                       // [7] the one-wave sweep's phases (printed; no kernel writes them now)
  // the trace phase: hit runs (cycles, records), the other accesses (cycles, count), then of the hit runs:
  // clock sums after the look-up, calls, clock sums at the start, after the row loop, after the stores; row updates
  PF_HR_CYCLES = 33, PF_HR_RECORDS, PF_ACC_CYCLES, PF_ACC_COUNT, PF_HR_T_LOOKUP, PF_HR_CALLS, PF_HR_T_START,
  PF_HR_T_LOOP, PF_HR_T_STORE, PF_HR_ROWS,
  PF_WALK_MAXPK = 46,                  // [stage] the most packets one run held
  PF_WALK_PAST64 = 48,                 // pipelined runs past 64 packets
  // prof_batch: requests by batch size bucket, [kind][8] (0 SELF, 1 injection, 2 walker); tail requests [kind]
  PF_BATCH = 50, PF_BATCH_KIND = 8, PF_BATCH_TAIL = 80,
  // a step's SELF phase in tiles with arrivals: cycles of [6] phases, the tiles; without: prologue cycles, the tiles
  PF_SELF_PHASE = 90, PF_SELF_TILES = 96, PF_NOSELF_PROLOGUE, PF_NOSELF_TILES,
  PF_ARM = 100, PF_ARM_HIT, PF_ARM_CONT, PF_ARM_MISS,   // the walkers' armed waits
  // per-launch maxima, in rings of PF_RING words from PF_RINGS on: ring r starts at PF_RINGS + r * PF_RING
  PF_RINGS = 1024, PF_RING = 65536,
  PF_R_STEP = PF_RINGS,                        // [L mod PF_RING] the slowest tile's cycles
  PF_R_WALK = PF_RINGS + 1 * PF_RING,          // [L mod PF_RING][stage] the slowest walker's cycles
  PF_R_STEP_REQ = PF_RINGS + 3 * PF_RING,      // [L mod PF_RING] a tile's most requests (SELF arrivals + sent)
  PF_R_WALK_REQ = PF_RINGS + 4 * PF_RING,      // [L mod PF_RING][stage] (printed; no kernel writes them now)
  PF_R_SHAPE = PF_RINGS + 6 * PF_RING,         // [L mod PF_SHAPES][4] the slowest tile's shape (k_c_step's end)
  PF_SHAPES = 16384,
  PF_WORDS = PF_RINGS + 8 * PF_RING            // the buffer
};
