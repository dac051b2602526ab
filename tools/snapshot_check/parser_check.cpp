// parser_check.cpp — the snapshot container's parser (graphite_amd/csrc/
// gg_snapshot.h) against valid, truncated and corrupted buffers, as a plain
// host program: build it with -fsanitize=address,undefined and run it
// (tests/test_snapshot_parser.py does).  Every buffer is a heap block of its
// exact size, so a read past it is a sanitizer report; whenever parse()
// accepts a buffer every byte of every section is read.
#include <stdio.h>
#include <stdlib.h>

#include "../../graphite_amd/csrc/gg_snapshot.h"

using namespace ggsnap;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// an exact-size heap copy, parsed; an accepted buffer is read through
static const char* parse_copy(const std::vector<uint8_t>& b, uint64_t n, uint64_t* sum)
{
  uint8_t* h = (uint8_t*)malloc(n ? n : 1);
  memcpy(h, b.data(), n);
  View v;
  const char* why = parse(h, n, &v);
  if (!why) {
    uint64_t t = 0;
    for (const Section& s : v.sec) {
      const uint8_t* d = v.data(s);
      for (uint64_t i = 0; i < s.bytes; ++i) t += d[i];
      if (s.kind == SK_PACKED)
        for (uint64_t r = 0; r < s.records; ++r) { uint64_t g; memcpy(&g, d + r * s.rec_bytes, 8); t += g; }
    }
    if (sum) *sum = t;
  }
  free(h);
  return why;
}

static std::vector<uint8_t> make_valid(uint64_t mtab_records = 2)
{
  Layout lay;
  lay.add("cfg", SK_DENSE, 0, 100, 0);              // (not a multiple of 8: padding follows)
  lay.add("empty", SK_DENSE, 0, 0, 0);
  lay.add("dir", SK_PACKED, 40, 40 * 7, 7);
  lay.add("a_long_name_1234", SK_DENSE, 0, 33, 0);  // 16 characters: cut to 15 + NUL
  lay.add("mtab", SK_PACKED, 16, 16 * mtab_records, mtab_records);
  const uint64_t total = lay.finish();
  std::vector<uint8_t> b(total, 0);
  for (const Section& s : lay.sec)
    for (uint64_t i = 0; i < s.bytes; ++i) b[s.off + i] = (uint8_t)(i * 7 + s.off);
  lay.write(b.data(), total);
  return b;
}

int main()
{
  const std::vector<uint8_t> ok = make_valid();
  uint64_t sum = 0;
  CHECK(parse_copy(ok, ok.size(), &sum) == nullptr);
  {
    View v;
    CHECK(parse(ok.data(), ok.size(), &v) == nullptr);
    CHECK(v.sec.size() == 5 && v.find("dir") && v.find("dir")->records == 7 && !v.find("nothing"));
    CHECK(v.find("a_long_name_123") != nullptr);
    CHECK(parse(nullptr, 10, &v) != nullptr);
    const std::vector<uint8_t> e = make_valid(0);       // an empty packed section is a valid one
    CHECK(parse_copy(e, e.size(), nullptr) == nullptr);
  }
  // truncated at every length, and longer than it says
  for (uint64_t n = 0; n < ok.size(); ++n) CHECK(parse_copy(ok, n, nullptr) != nullptr);
  {
    std::vector<uint8_t> b = ok;
    b.resize(ok.size() + 8, 0);
    CHECK(parse_copy(b, b.size(), nullptr) != nullptr);
  }
  // every header and table field overwritten with small, huge and wrapping values
  const uint64_t vals[] = {0, 1, 7, 8, 0x7FFFFFFFull, 0xFFFFFFFFull, 0x100000000ull, 1ull << 40, 1ull << 63,
                           ~0ull, ~0ull - 7, ~0ull - 47};
  const uint64_t table_end = sizeof(Header) + 5 * sizeof(Section);
  for (uint64_t off = 0; off + 4 <= table_end; off += 4)
    for (uint64_t val : vals)
      for (int width = 4; width <= 8; width += 4) {
        if (off + width > table_end) continue;
        std::vector<uint8_t> b = ok;
        memcpy(b.data() + off, &val, width);
        // a changed size, offset, kind or count never passes (names may change freely)
        bool changed = false;
        for (uint64_t i = off; i < off + width; ++i) {
          const bool name = i >= sizeof(Header) && (i - sizeof(Header)) % sizeof(Section) < 16;
          changed = changed || (!name && b[i] != ok[i]);
        }
        const char* why = parse_copy(b, b.size(), nullptr);
        if (changed) CHECK(why != nullptr);
      }
  // a payload byte flipped: the checksum
  for (uint64_t i = table_end; i < ok.size(); i += 13) {
    std::vector<uint8_t> b = ok;
    b[i] ^= 0x40;
    CHECK(parse_copy(b, b.size(), nullptr) != nullptr);
  }
  // random corruption of the header and the table (the checksum does not cover them)
  uint64_t lcg = 12345;
  for (int it = 0; it < 20000; ++it) {
    std::vector<uint8_t> b = ok;
    const int flips = 1 + it % 4;
    for (int f = 0; f < flips; ++f) {
      lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
      b[(lcg >> 33) % table_end] = (uint8_t)(lcg >> 20);
    }
    (void)parse_copy(b, b.size(), nullptr);           // must not read out of bounds, whatever it answers
  }
  printf(failures ? "parser_check: %d failures\n" : "parser_check: ok\n", failures);
  return failures ? 1 : 0;
}
