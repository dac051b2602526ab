// window_check.cpp — the reader of a windowed run's `win` section
// (graphite_amd/csrc/gg_snapshot_win.h, what gg_window_snapshot_state calls)
// against valid and broken containers, as a plain host program: build it with
// -fsanitize=address,undefined and run it (tests/test_window_snapshot_parser.py
// does).  Every container is built with ggsnap::Layout and handed over as a
// heap block of its exact size, and the output arrays are heap blocks of
// exactly num_tiles entries, so a read or a write past either is a sanitizer
// report.  A refused buffer must leave the arrays as they were.
#include <stdio.h>
#include <stdlib.h>

#include "../../graphite_amd/csrc/gg_snapshot_win.h"

using namespace ggsnap;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static WinRec rec_of(uint32_t t)
{
  const bool fin = t % 3 == 2;
  return WinRec{100 + 7ull * t, fin ? 1ull : 0ull, fin ? 0ull : (0x4000000ull * (t + 1)) | 0x40, fin ? 0ull : (t & 1) | 0x80000000ull};
}

// a container with a few of the sections a snapshot carries; win_tiles < 0: no win section
static std::vector<uint8_t> make(int win_tiles, uint32_t tiles_in_recs = 0)
{
  Layout lay;
  lay.add("cfg", SK_DENSE, 0, 100, 0);
  lay.add("ts", SK_DENSE, 0, 64 * 5, 0);
  lay.add("dir", SK_PACKED, 40, 40 * 3, 3);
  size_t w = 0;
  if (win_tiles >= 0) w = lay.add(kWinSection, SK_DENSE, 0, sizeof(WinRec) * (uint64_t)win_tiles, 0);
  const uint64_t total = lay.finish();
  std::vector<uint8_t> b(total, 0);
  for (size_t i = 0; i < lay.sec.size(); ++i)
    for (uint64_t k = 0; k < lay.sec[i].bytes; ++k) b[lay.sec[i].off + k] = (uint8_t)(k * 5 + i);
  if (win_tiles >= 0) {
    memset(b.data() + lay.sec[w].off, 0, lay.sec[w].bytes);
    for (uint32_t t = 0; t < tiles_in_recs && t < (uint32_t)win_tiles; ++t) {
      const WinRec r = rec_of(t);
      memcpy(b.data() + lay.sec[w].off + (uint64_t)t * sizeof(WinRec), &r, sizeof(r));
    }
  }
  lay.write(b.data(), total);
  return b;
}

// the first n bytes as an exact-size heap block, read for T tiles into exact-size arrays
static const char* read_copy(const std::vector<uint8_t>& b, uint64_t n, uint32_t T, std::vector<uint64_t>* consumed,
                             std::vector<uint8_t>* finished, bool want_c = true, bool want_f = true)
{
  uint8_t* h = (uint8_t*)malloc(n ? n : 1);
  memcpy(h, b.data(), n);
  uint64_t* c = (uint64_t*)malloc(sizeof(uint64_t) * (T ? T : 1));
  uint8_t* f = (uint8_t*)malloc(T ? T : 1);
  for (uint32_t t = 0; t < T; ++t) { c[t] = 0xC0FFEEull; f[t] = 0xEE; }
  const char* why = win_read(h, n, T, want_c ? c : nullptr, want_f ? f : nullptr);
  if (consumed) consumed->assign(c, c + T);
  if (finished) finished->assign(f, f + T);
  free(h); free(c); free(f);
  return why;
}

static bool untouched(const std::vector<uint64_t>& c, const std::vector<uint8_t>& f)
{
  for (uint64_t x : c) if (x != 0xC0FFEEull) return false;
  for (uint8_t x : f) if (x != 0xEE) return false;
  return true;
}

int main()
{
  const uint32_t T = 7;
  std::vector<uint64_t> c;
  std::vector<uint8_t> f;
  // a valid win section: every verdict and every entry
  const std::vector<uint8_t> ok = make((int)T, T);
  CHECK(read_copy(ok, ok.size(), T, &c, &f) == nullptr);
  for (uint32_t t = 0; t < T; ++t) CHECK(c[t] == rec_of(t).consumed && f[t] == rec_of(t).finished);
  // either array may be null; the other is still filled
  CHECK(read_copy(ok, ok.size(), T, &c, &f, false, true) == nullptr);
  for (uint32_t t = 0; t < T; ++t) CHECK(c[t] == 0xC0FFEEull && f[t] == rec_of(t).finished);
  CHECK(read_copy(ok, ok.size(), T, &c, &f, true, false) == nullptr);
  for (uint32_t t = 0; t < T; ++t) CHECK(c[t] == rec_of(t).consumed && f[t] == 0xEE);
  CHECK(read_copy(ok, ok.size(), T, nullptr, nullptr, false, false) == nullptr);
  {
    View v;
    const uint8_t* p = nullptr;
    CHECK(parse(ok.data(), ok.size(), &v) == nullptr && win_section(v, T, &p) == nullptr && p == v.data(*v.find(kWinSection)));
  }
  // no win section: the snapshot of an ordinary run
  {
    const std::vector<uint8_t> b = make(-1);
    const char* why = read_copy(b, b.size(), T, &c, &f);
    CHECK(why != nullptr && strstr(why, "gg_coherent_restore") != nullptr && untouched(c, f));
  }
  // a win section of the wrong size for num_tiles, both ways
  for (uint32_t other : {T - 1, T + 1, 1u, 64u}) {
    const char* why = read_copy(ok, ok.size(), other, &c, &f);
    CHECK(why != nullptr && strstr(why, "num_tiles") != nullptr && untouched(c, f));
  }
  {
    const std::vector<uint8_t> b = make(0);             // an empty win section
    CHECK(read_copy(b, b.size(), T, &c, &f) != nullptr && untouched(c, f));
  }
  // num_tiles = 0
  CHECK(read_copy(ok, ok.size(), 0, &c, &f) != nullptr);
  {
    const std::vector<uint8_t> b = make(0);
    CHECK(read_copy(b, b.size(), 0, &c, &f) != nullptr);
  }
  // truncated at every length (the table included), and longer than it says
  for (uint64_t n = 0; n < ok.size(); ++n) CHECK(read_copy(ok, n, T, &c, &f) != nullptr && untouched(c, f));
  {
    std::vector<uint8_t> b = ok;
    b.resize(ok.size() + 8, 0);
    CHECK(read_copy(b, b.size(), T, &c, &f) != nullptr && untouched(c, f));
  }
  // a section past the buffer: the win section's offset and size overwritten
  {
    const uint64_t ent = sizeof(Header) + 3 * sizeof(Section);
    const uint64_t vals[] = {0, 8, 1ull << 40, ~0ull - 7, ~0ull, ok.size(), ok.size() - 8};
    for (uint64_t field : {32ull, 24ull})                 // bytes, off
      for (uint64_t val : vals) {
        std::vector<uint8_t> b = ok;
        uint64_t was;
        memcpy(&was, b.data() + ent + field, 8);
        if (was == val) continue;
        memcpy(b.data() + ent + field, &val, 8);
        CHECK(read_copy(b, b.size(), T, &c, &f) != nullptr && untouched(c, f));
      }
    std::vector<uint8_t> b = ok;                        // the section count one more than the table holds
    uint32_t ns = 5;
    memcpy(b.data() + 12, &ns, 4);
    CHECK(read_copy(b, b.size(), T, &c, &f) != nullptr && untouched(c, f));
  }
  // a bad checksum: a payload byte flipped, in the win section and before it
  {
    View v;
    CHECK(parse(ok.data(), ok.size(), &v) == nullptr);
    const uint64_t table_end = sizeof(Header) + v.sec.size() * sizeof(Section);
    for (uint64_t i = table_end; i < ok.size(); i += 11) {
      std::vector<uint8_t> b = ok;
      b[i] ^= 0x10;
      const char* why = read_copy(b, b.size(), T, &c, &f);
      CHECK(why != nullptr && strstr(why, "checksum") != nullptr && untouched(c, f));
    }
  }
  // records that no snapshot holds (checksum right): a flag past 1, a meta word past 32 bits, a finished tile with a record
  for (int k = 0; k < 3; ++k) {
    Layout lay;
    lay.add(kWinSection, SK_DENSE, 0, sizeof(WinRec) * T, 0);
    const uint64_t total = lay.finish();
    std::vector<uint8_t> b(total, 0);
    WinRec r = k == 0 ? WinRec{5, 2, 0, 0} : k == 1 ? WinRec{5, 0, 64, 1ull << 32} : WinRec{5, 1, 64, 0};
    memcpy(b.data() + lay.sec[0].off + 3 * sizeof(WinRec), &r, sizeof(r));
    lay.write(b.data(), total);
    CHECK(read_copy(b, b.size(), T, &c, &f) != nullptr && untouched(c, f));
  }
  printf(failures ? "window_check: %d failures\n" : "window_check: ok\n", failures);
  return failures ? 1 : 0;
}
