// devmem_check.cpp — the two owners of device memory (graphite_amd/csrc/
// gg_devmem.h: gg_arena, gg_dbuf and gg_reserve_all) over a counting host
// allocator that can be told to fail its k-th call, as a plain host program:
// build it with -fsanitize=address,undefined and run it
// (tests/test_devmem.py does).  Every block is a malloc block of its exact
// size, so a double free or a use after free is also a sanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <map>

#define GG_DEVMEM_ALLOCATOR
#include "../../include/graphite_gpu.h"

// the substituted allocator: live blocks with their sizes, call counts, the
// frees of an address that is not live, and a countdown to a failing call
struct Counting {
  std::map<void*, size_t> live;
  uint64_t allocs = 0, handed = 0, frees = 0, bad_frees = 0;   // handed: the alloc calls that succeeded
  uint64_t fail_in = 0;                // k: the k-th alloc call from now fails (0: none)
  void fail_at(uint64_t k) { fail_in = k; }
  uint64_t calls() const { return allocs + frees; }
};
static Counting G;

struct gg_mem_device {
  static gg_status alloc(void** p, size_t bytes)
  {
    ++G.allocs;
    if (G.fail_in && --G.fail_in == 0) return GG_ERR_HIP;
    *p = malloc(bytes ? bytes : 1);
    G.live[*p] = bytes;
    ++G.handed;
    return GG_OK;
  }
  static void release(void* p)
  {
    ++G.frees;
    auto it = G.live.find(p);
    if (it == G.live.end()) { ++G.bad_frees; return; }   // freed twice, or never allocated
    G.live.erase(it);
    free(p);
  }
};
struct gg_mem_pinned : gg_mem_device {};

#include "../../graphite_amd/csrc/gg_devmem.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

// empty, or a live block of exactly capacity() elements
template <class B, class T = std::remove_pointer_t<decltype(std::declval<B>().get())>>
static bool sound(const B& b)
{
  if (!b.get()) return b.capacity() == 0;
  auto it = G.live.find((void*)b.get());
  return it != G.live.end() && b.capacity() != 0 && it->second == b.capacity() * sizeof(T);
}

struct Group {        // five arrays of one capacity, as the packet arrays of the NoC batch
  gg_dbuf<uint64_t> a, b;
  gg_dbuf<uint32_t> c, d;
  gg_dbuf<uint8_t> e;
  gg_status grow(uint64_t n) { return gg_reserve_all(n, n + n / 4 + 1024, a, b, c, d, e); }
  bool all_sound() const { return sound(a) && sound(b) && sound(c) && sound(d) && sound(e); }
  bool all_at(uint64_t cap) const
  {
    return a.capacity() == cap && b.capacity() == cap && c.capacity() == cap && d.capacity() == cap && e.capacity() == cap;
  }
};

static void group_failures()
{
  for (int regrow = 0; regrow < 2; ++regrow)
    for (uint64_t k = 1; k <= 5; ++k) {
      {
        Group g;
        uint64_t n = 200;
        if (regrow) {                                  // from a non-empty state
          CHECK(g.grow(n) == GG_OK);
          CHECK(g.all_sound() && g.all_at(200 + 50 + 1024));
          n = 3000;                                    // above 200 + 50 + 1024: every member is short
        }
        G.fail_at(k);
        CHECK(g.grow(n) == GG_ERR_HIP);
        CHECK(G.fail_in == 0);                         // (the k-th call was reached)
        CHECK(g.all_sound());
        CHECK(!g.all_at(n + n / 4 + 1024));
        CHECK(G.bad_frees == 0);
        // the members ahead of the failing one hold the new capacity, the rest are empty
        const uint64_t caps[5] = {g.a.capacity(), g.b.capacity(), g.c.capacity(), g.d.capacity(), g.e.capacity()};
        for (uint64_t i = 0; i < 5; ++i) CHECK(caps[i] == (i + 1 < k ? n + n / 4 + 1024 : 0));
        CHECK(g.grow(n) == GG_OK);                     // the retry
        CHECK(g.all_sound() && g.all_at(n + n / 4 + 1024));
        CHECK(G.live.size() == 5);
        // the blocks can be written over their whole length
        for (uint64_t i = 0; i < g.a.capacity(); ++i) { g.a.get()[i] = i; g.e.get()[i] = (uint8_t)i; }
        const uint64_t before = G.calls();
        CHECK(g.grow(n) == GG_OK && g.grow(1) == GG_OK && g.grow(g.a.capacity()) == GG_OK);
        CHECK(G.calls() == before);                    // room already: no allocator call
      }
      CHECK(G.live.empty());                           // after destruction
      CHECK(G.bad_frees == 0);
    }
}

static void single_buffer()
{
  {
    gg_dbuf<uint32_t> b;
    CHECK(b.get() == nullptr && b.capacity() == 0 && sound(b));
    uint64_t before = G.calls();
    CHECK(b.reserve(0) == GG_OK && b.reserve(0, 64) == GG_OK);
    CHECK(G.calls() == before && !b.get());            // need 0 <= capacity 0
    CHECK(b.reserve(10, 12) == GG_OK);
    CHECK(sound(b) && b.capacity() == 12);
    uint32_t* const p = b.get();
    CHECK(static_cast<uint32_t*>(b) == p);             // the conversion the launch sites use
    before = G.calls();
    CHECK(b.reserve(12, 1000) == GG_OK && b.reserve(1) == GG_OK);
    CHECK(G.calls() == before && b.get() == p && b.capacity() == 12);
    CHECK(b.reserve(13, 20) == GG_OK);                 // short by one: freed, then allocated
    CHECK(G.calls() == before + 2 && sound(b) && b.capacity() == 20);
    G.fail_at(1);
    CHECK(b.reserve(21) == GG_ERR_HIP);
    CHECK(!b.get() && b.capacity() == 0 && G.live.empty());   // a failure leaves it empty
    CHECK(b.reserve(21) == GG_OK && sound(b) && b.capacity() == 21);
    // move-only: the source is left empty, the target's old block is freed
    gg_dbuf<uint32_t> c(std::move(b));
    CHECK(!b.get() && b.capacity() == 0 && sound(c) && c.capacity() == 21);
    gg_dbuf<uint32_t> d;
    CHECK(d.reserve(5) == GG_OK);
    d = std::move(c);
    CHECK(!c.get() && sound(d) && d.capacity() == 21 && G.live.size() == 1);
    d.reset();
    CHECK(!d.get() && G.live.empty());
    gg_dbuf<uint64_t, gg_mem_pinned> h;                // the pinned flavour is the same type over the other pair
    CHECK(h.reserve(7) == GG_OK && sound(h));
  }
  CHECK(G.live.empty() && G.bad_frees == 0);
}

// a call-local temporary and an early return, as gg_cache_quartet's block
static gg_status temporary(bool fail_later, const void** seen)
{
  gg_dbuf<uint64_t> tmp;
  if (gg_status st = tmp.reserve(3)) return st;
  *seen = tmp.get();
  if (fail_later) return GG_ERR_STATE;                 // (a failed copy or launch)
  return GG_OK;
}

static void temporaries()
{
  const void* seen = nullptr;
  CHECK(temporary(true, &seen) == GG_ERR_STATE && seen && G.live.empty());
  CHECK(temporary(false, &seen) == GG_OK && G.live.empty());
  G.fail_at(1);
  seen = nullptr;
  CHECK(temporary(false, &seen) == GG_ERR_HIP && !seen && G.live.empty());
  CHECK(G.bad_frees == 0);
}

static void arena()
{
  const int N = 6;
  for (uint64_t k = 1; k <= (uint64_t)N; ++k) {
    uint64_t* p[N];
    uint64_t sentinel = 0;
    {
      gg_arena m;
      for (int i = 0; i < N; ++i) p[i] = &sentinel;
      G.fail_at(k);
      gg_status st = GG_OK;
      int done = 0;
      for (; done < N && st == GG_OK; ++done) st = m.alloc(&p[done], (uint64_t)done);   // (0 elements: one is allocated)
      CHECK(st == GG_ERR_HIP && (uint64_t)done == k);
      for (uint64_t i = 0; i < (uint64_t)N; ++i)
        if (i + 1 < k) CHECK(G.live.count(p[i]) == 1 && G.live[p[i]] == 8 * (i ? i : 1));
        else CHECK(p[i] == &sentinel);                 // set on success only
      CHECK(G.live.size() == k - 1);
      uint32_t* q = nullptr;
      CHECK(m.alloc(&q, 9) == GG_OK && G.live.count(q) == 1);   // the arena goes on after a failure
      if (k == 1) { m.clear(); CHECK(G.live.empty()); CHECK(m.alloc(&q, 2) == GG_OK); }   // cleared and used again
    }
    CHECK(G.live.empty() && G.bad_frees == 0);
  }
}

int main()
{
  group_failures();
  single_buffer();
  temporaries();
  arena();
  // every block that was handed out was freed exactly once
  CHECK(G.live.empty() && G.bad_frees == 0 && G.handed == G.frees);
  if (failures) { printf("devmem_check: %d failure(s)\n", failures); return 1; }
  printf("devmem_check: ok (%llu allocator calls)\n", (unsigned long long)G.calls());
  return 0;
}
