// gg_snapshot_win.h — the `win` section of a windowed run's snapshot
// (gg_coherent_window_snapshot / _window_restore): one
// record per tile, by tile number.  Plain C++ with no HIP calls, like the
// container (gg_snapshot.h): the bytes may come from a file, and a program
// that only wants to know where each tile's next window begins
// (gg_window_snapshot_state) needs nothing else.
//
//   WinRec { consumed, finished, addr, meta }
//
// consumed: the records the tile has passed since begin, so its next window
// begins at record `consumed` of its trace.  finished: 1 when the tile has
// passed the last record of its trace.  addr / meta: the record an unfinished
// tile stands on (meta in the low 32 bits; both 0 for a finished tile), which
// the first record of the window it is restored with must equal.
//
// Nothing here depends on where the windows were cut: no final flag, no
// guard, no index into a window's arrays.
#pragma once
#include "gg_snapshot.h"

namespace ggsnap {

constexpr const char* kWinSection = "win";
struct WinRec { uint64_t consumed, finished, addr, meta; };
static_assert(sizeof(WinRec) == 32, "the win section's layout is fixed");

// nullptr and *recs = the section's num_tiles records (unaligned: memcpy), or
// what is wrong with it; v is a parsed container
inline const char* win_section(const View& v, uint32_t num_tiles, const uint8_t** recs)
{
  if (num_tiles == 0) return "num_tiles is 0";
  const Section* s = v.find(kWinSection);
  if (!s) return "no win section: not the snapshot of a run fed in windows (gg_coherent_restore takes it)";
  if (s->kind != SK_DENSE) return "win section: kind";
  if (s->bytes != (uint64_t)num_tiles * sizeof(WinRec)) return "win section: its size is not num_tiles records";
  const uint8_t* p = v.data(*s);
  for (uint32_t t = 0; t < num_tiles; ++t) {
    WinRec r;
    memcpy(&r, p + (uint64_t)t * sizeof(WinRec), sizeof(r));
    if (r.finished > 1 || (r.meta >> 32)) return "win section: a record's flag or meta word";
    if (r.finished && (r.addr || r.meta)) return "win section: a finished tile with a record to stand on";
  }
  if (recs) *recs = p;
  return nullptr;
}

// The container parsed (bounds, checksum) and its win section read:
// consumed[num_tiles] and finished[num_tiles], either may be null.  nullptr,
// or the reason; the arrays are written only on success.
inline const char* win_read(const void* buf, uint64_t bytes, uint32_t num_tiles, uint64_t* consumed, uint8_t* finished)
{
  View v;
  if (const char* why = parse(buf, bytes, &v)) return why;
  const uint8_t* p = nullptr;
  if (const char* why = win_section(v, num_tiles, &p)) return why;
  for (uint32_t t = 0; t < num_tiles; ++t) {
    WinRec r;
    memcpy(&r, p + (uint64_t)t * sizeof(WinRec), sizeof(r));
    if (consumed) consumed[t] = r.consumed;
    if (finished) finished[t] = (uint8_t)r.finished;
  }
  return nullptr;
}

}  // namespace ggsnap
