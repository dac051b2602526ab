// gg_snapshot.h — the container of a coherent run's snapshot
// (gg_coherent_snapshot / gg_coherent_restore): header, section
// table, payload.  Plain C++ with no HIP calls: the bytes may come from a file,
// so everything is read with memcpy (no alignment assumed) and every offset
// and size is checked against the buffer before anything is looked at.
//
//   Header   { magic, version, sections, total bytes, payload checksum }
//   Section  { name[16], kind, record bytes, offset, bytes, records } x sections
//   payload  sections at 8-byte aligned offsets, in table order
//
// kind SK_DENSE: `bytes` of an array as it lies in memory (records = 0).
// kind SK_PACKED: `records` records of `rec_bytes` each (bytes = their
// product): {slot index, the slot's words}, in slot order — the arrays whose
// unused slots are not worth (or not fit) to copy.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

namespace ggsnap {

constexpr uint64_t kMagic = 0x3130504E53474721ull;   // "!GGSNP01"
constexpr uint32_t kVersion = 1;
constexpr uint32_t kMaxSections = 256;
enum { SK_DENSE = 0, SK_PACKED = 1 };

struct Header { uint64_t magic; uint32_t version, sections; uint64_t total, checksum; };
struct Section { char name[16]; uint32_t kind, rec_bytes; uint64_t off, bytes, records; };
static_assert(sizeof(Header) == 32 && sizeof(Section) == 48, "the container's layout is fixed");

inline uint64_t align8(uint64_t v) { return (v + 7) & ~7ull; }

// a multiply-xor hash over the payload: four independent lanes of 8 bytes a
// round (one lane's multiply chain runs at ~4 GB/s; a snapshot is 100 MB and
// more), folded at the end; the tail byte-wise
inline uint64_t checksum(const uint8_t* p, uint64_t n)
{
  uint64_t h[4] = {0x9E3779B97F4A7C15ull, 0xC2B2AE3D27D4EB4Full, 0x165667B19E3779F9ull, 0x27D4EB2F165667C5ull};
  uint64_t i = 0;
  for (; i + 32 <= n; i += 32) {
    uint64_t w[4];
    memcpy(w, p + i, 32);
    for (int k = 0; k < 4; ++k) { h[k] = (h[k] ^ w[k]) * 0xFF51AFD7ED558CCDull; h[k] ^= h[k] >> 32; }
  }
  uint64_t r = n;
  for (int k = 0; k < 4; ++k) { r = (r ^ h[k]) * 0xC4CEB9FE1A85EC53ull; r ^= r >> 29; }
  for (; i < n; ++i) { r = (r ^ p[i]) * 0x100000001B3ull; }
  return r;
}

struct View {
  const uint8_t* base = nullptr;
  uint64_t bytes = 0;
  Header h{};
  std::vector<Section> sec;
  const Section* find(const char* name) const
  {
    for (const Section& s : sec)
      if (strncmp(s.name, name, sizeof(s.name)) == 0) return &s;
    return nullptr;
  }
  const uint8_t* data(const Section& s) const { return base + s.off; }
};

// nullptr, or what is wrong with the buffer.  After success every section of
// v->sec lies inside [table end, bytes) and a packed section's records fill it.
inline const char* parse(const void* buf, uint64_t bytes, View* v, bool verify_checksum = true)
{
  if (!buf || !v) return "NULL buffer";
  if (bytes < sizeof(Header)) return "shorter than the header";
  const uint8_t* p = (const uint8_t*)buf;
  Header h;
  memcpy(&h, p, sizeof(h));
  if (h.magic != kMagic) return "not a snapshot (magic)";
  if (h.version != kVersion) return "unknown format version";
  if (h.sections == 0 || h.sections > kMaxSections) return "section count out of range";
  const uint64_t table_end = sizeof(Header) + (uint64_t)h.sections * sizeof(Section);
  if (h.total != bytes) return h.total > bytes ? "truncated buffer" : "buffer longer than the snapshot";
  if (table_end > bytes) return "section table past the buffer";
  v->base = p; v->bytes = bytes; v->h = h;
  v->sec.resize(h.sections);
  memcpy(v->sec.data(), p + sizeof(Header), (size_t)h.sections * sizeof(Section));
  uint64_t at = table_end;
  for (const Section& s : v->sec) {
    if (memchr(s.name, 0, sizeof(s.name)) == nullptr || s.name[0] == 0) return "section name";
    if (s.kind != SK_DENSE && s.kind != SK_PACKED) return "section kind";
    if (s.off & 7) return "section offset not aligned";
    if (s.off != at) return "section offset out of order";
    if (s.bytes > bytes || s.off > bytes - s.bytes) return "section past the buffer";
    if (s.kind == SK_PACKED) {
      if (s.rec_bytes == 0 || (s.rec_bytes & 7)) return "packed section: record size";
      if (s.records > s.bytes / s.rec_bytes || s.records * s.rec_bytes != s.bytes) return "packed section: record count";
    } else if (s.records != 0 || s.rec_bytes != 0) return "dense section with records";
    at = align8(s.off + s.bytes);
    if (at < s.off) return "section past the buffer";
  }
  if (at != bytes) return "payload size disagrees with the section table";
  if (verify_checksum && checksum(p + table_end, bytes - table_end) != h.checksum) return "payload checksum";
  return nullptr;
}

// ---- writing: the table is laid out first (sizes), then filled ---------------
struct Layout {
  std::vector<Section> sec;
  uint64_t add(const char* name, uint32_t kind, uint32_t rec_bytes, uint64_t bytes, uint64_t records)
  {
    Section s{};
    strncpy(s.name, name, sizeof(s.name) - 1);
    s.kind = kind; s.rec_bytes = rec_bytes; s.bytes = bytes; s.records = records;
    sec.push_back(s);
    return sec.size() - 1;
  }
  // assigns the offsets; the total size
  uint64_t finish()
  {
    uint64_t at = sizeof(Header) + sec.size() * sizeof(Section);
    for (Section& s : sec) { s.off = at; at = align8(at + s.bytes); }
    return at;
  }
  // header and table into buf (after the payload is in place: the checksum)
  void write(uint8_t* buf, uint64_t total) const
  {
    const uint64_t table_end = sizeof(Header) + sec.size() * sizeof(Section);
    memcpy(buf + sizeof(Header), sec.data(), sec.size() * sizeof(Section));
    Header h{kMagic, kVersion, (uint32_t)sec.size(), total, checksum(buf + table_end, total - table_end)};
    memcpy(buf, &h, sizeof(h));
  }
};

}  // namespace ggsnap
