// gg_coh_window.h — a coherent run fed its trace in windows:
// the launchers of the hand-over and window-state kernels (gg_coh_window.hip).
// The host side of gg_coherent_begin_window / _next_window / _window_state
// follows the kernels there.
#pragma once
#include "gg_coh_dev.h"

namespace ggc {

// what the hand-over kernel found wrong, per bit (checked before anything changes)
enum { WB_EMPTY = 1,      // an unfinished tile's window holds no record
       WB_RECORD = 2,     // its first record is not the record the tile stands on (addr or meta)
       WB_FINAL = 4,      // a final tile made non-final, or its remaining records changed in number
       WB_FINISHED = 8,   // a finished tile's range is not empty
       WB_STATE = 16 };   // a tile off the end of a window (the run has failed)
// bad[0]: the WB_* bits, bad[1]: the first offending tile + 1 (the least)

// mode 0: the first window of a begun run (the tiles stand at offs[tile]):
// final flags, guards, the horizon.  mode 1: check a next window against the
// tiles' state, nothing written but bad[].  mode 2: install it (rebase rec /
// rec_end, final flags, consumed counts, guards, the horizon).  addr / meta
// are the new window's arrays; offs [T + 1] and fin [T] (or null) on the device.
void launch_window_install(const CP& P, const CS& S, const uint64_t* addr, const uint32_t* meta, const uint64_t* offs,
                           const uint8_t* fin, int mode, uint32_t* bad, hipStream_t s);
// consumed [T] and min_records [T] (device; zeros for tiles not owned)
void launch_window_state(const CP& P, const CS& S, uint64_t* consumed, uint64_t* min_records, hipStream_t s);

// A windowed run's snapshot (gg_coherent_window_snapshot).  recs [T][4]: a
// tile's {consumed, finished, addr, meta of the record it stands on} by tile
// number (ggsnap::WinRec); ts_out [L]: S.ts with rec = consumed and rec_end =
// 0.  The run's own state is read, never written.
void launch_window_gather(const CP& P, const CS& S, TileSt* ts_out, uint64_t* recs, hipStream_t s);
// Its restore (gg_coherent_window_restore); recs as above, from the snapshot.
// phase 0, before anything is changed: win's ranges against recs, the verdict
// in bad[] as mode 1 leaves it (no tile state is read).  phase 1, once the
// reset and the snapshot's arrays are in place (S.ts canonical, S.win bound,
// its header ~0): rec / rec_end onto win's arrays, the WN_* words, the horizon.
void launch_window_restore(const CP& P, const CS& S, const uint64_t* addr, const uint32_t* meta, const uint64_t* offs,
                           const uint8_t* fin, const uint64_t* recs, int phase, uint32_t* bad, hipStream_t s);

}  // namespace ggc
