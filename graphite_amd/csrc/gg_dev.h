// gg_dev.h — device-side building blocks shared by the NoC (gg_noc.hip) and
// coherent (gg_coherent.hip) paths: the QueueModelHistoryTree restatement,
// the time conversions and the closed-form EMesh routes.
#pragma once
#include "gg_internal.h"

namespace gg {

// ---------------------------------------------------------------------------
// Queue models (QueueModel::create, queue_model.cc:19-39).  One storage
// layout for all three: HQueue + max_size 16-byte HNode slots.
//   history_tree (queue_model_history_tree.cc:44-167 over interval_tree.cc):
//     the free intervals sorted by start in a circular list of max_size
//     slots (interval i at slot (head + i) mod max_size), so the pruning of
//     the oldest interval is head + 1 and the usual update — at the newest
//     interval, the packets of a port arriving in time order — touches one
//     slot.  The reference keeps
//     them in an AVL tree and finds the interval with searchTree
//     (interval_tree.cc:366-394); the free intervals are disjoint and, since
//     every processing time and min_processing_time is >= 1 (router queues 1,
//     router_model.cc:23-27; DRAM 13, dram_perf_model.cc:48,92), separated by
//     at least one busy cycle and at least min_processing_time long.  For such
//     a set searchTree returns the FIRST interval (lowest start) that either
//     contains [t, t+p] or starts after t with length >= p, whatever the tree
//     shape: a left subtree it skips (t + p >= node start) holds only
//     intervals that end at or before the node's start, so none contains
//     [t, t+p] and none starting after t is long enough.  search(0, 1) is
//     then nd[0] (the min-key node the pruning removes, :52-56).  The
//     outputs (delays, analytical count, utilization) are those of the AVL
//     (tests/test_queue_flat.py checks 600k random requests against the
//     oracle's AVL restatement; the reference fixtures run on the GPU).
//   history_list (queue_model_history_list.cc:40-134): nd[0..size) in list order;
//   basic (queue_model_basic.cc:34-61): the MovingAverage window
//     (moving_average.h, window + 1 slots) as raw u64 words over nd[].
// ---------------------------------------------------------------------------
struct HNode { uint64_t first, second; };
struct HQueue {
  uint32_t size; uint32_t max_size; uint32_t type, aux;   // GG_QM_*; list: no-interleaving flag; basic: basic_moving_avg
  uint64_t sig_sq, sig, n, newest;                  // QueueModelMG1: sums of p^2 and p (integers, see mg1_queue_delay)
  uint64_t analytical;                              // _total_requests_using_analytical_model
  uint64_t util, last_req, total_req;               // QueueModel utilization counters
  uint32_t front, back;                             // basic: ModuloNum window ends (modulo window + 1)
  double mean;                                      // basic: MovingArithmeticMean::_arithmetic_mean
  uint64_t qtime;                                   // basic: QueueModelBasic::_queue_time
  uint32_t head, pad;                               // history_tree: slot of interval 0 (circular list)
};
static_assert(sizeof(HQueue) % 16 == 0 && sizeof(HNode) == 16, "16-byte queue images");

// the model-specific parameter of a queue of type `type` (gg_config fields)
__host__ __device__ inline uint32_t hq_aux(uint32_t type, uint32_t basic_moving_avg, uint32_t list_no_interleaving)
{
  return type == GG_QM_BASIC ? basic_moving_avg : list_no_interleaving;
}
__host__ __device__ inline uint32_t hq_window(uint32_t aux) { return (aux & 0xFFFFu) ? (aux & 0xFFFFu) : 64u; }

// host-side validation of a queue model configuration
inline gg_status gg_check_queue_model(uint32_t type, uint32_t aux, uint32_t max_size)
{
  if (type > GG_QM_BASIC) return gg_fail(GG_ERR_INVALID, "unknown queue model type");
  if (max_size < 2) return gg_fail(GG_ERR_UNSUPPORTED, "max_list_size below 2");
  if (type == GG_QM_BASIC) {
    if ((aux >> 16) == GG_MAVG_GEOMETRIC_MEAN) return gg_fail(GG_ERR_UNSUPPORTED, "geometric_mean moving average");
    if ((aux >> 16) > GG_MAVG_GEOMETRIC_MEAN) return gg_fail(GG_ERR_INVALID, "unknown moving average type");
    if (hq_window(aux) + 1 > 2 * max_size)
      return gg_fail(GG_ERR_UNSUPPORTED, "moving_avg_window_size + 1 exceeds 2 * max_list_size queue words");
  }
  return GG_OK;
}

// QueueModel{HistoryTree,HistoryList,Basic} constructors on one queue's storage
__device__ inline void hq_init(HQueue* q, HNode* N, uint32_t max_size, uint32_t type, uint32_t aux)
{
  HQueue Q{};
  Q.max_size = max_size;
  Q.type = type;
  Q.aux = aux;
  if (type == GG_QM_BASIC) {
    uint64_t* w = reinterpret_cast<uint64_t*>(N);
    for (uint32_t j = 0; j <= hq_window(aux); ++j) w[j] = 0;   // _num_list.resize(window + 1)
  } else {
    N[0].first = 0; N[0].second = ~0ull;            // history_tree: allocateNode(PAIR(0, UINT64_MAX));
    Q.size = 1;                                     // history_list: push_back(make_pair(0, UINT64_MAX))
  }
  *q = Q;
}

// One wave's lane id and wave-level ordering of LDS accesses between lanes.
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ void wave_sync()
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint64_t ballot64(bool b) { return __ballot(b); }

// QueueModelMG1::computeQueueDelay (queue_model_m_g_1.cc).  The reference
// accumulates _service_time_sum(2) in doubles; every term is an integer
// processing time, so while the sums stay below 2^53 the double sums are the
// exact integers kept here (mg1_update flags GG_DERR_RANGE beyond).
__device__ __forceinline__ uint64_t mg1_queue_delay(uint64_t n, uint64_t newest, uint64_t ssq, uint64_t ss)
{
  if (n == 0) return 0;
  const double sig_sq = (double)ssq, sig = (double)ss;
  double variance = (sig_sq / n) - ((sig / n) * (sig / n));
  double service_rate = 1.0 / (sig / n);
  double arrival_rate = ((double)n) / newest;
  if (arrival_rate >= service_rate) arrival_rate = 0.999 * service_rate;
  return (uint64_t)ceil(0.5 * service_rate * arrival_rate * ((1 / (service_rate * service_rate)) + variance) /
                        (service_rate - arrival_rate));
}
constexpr uint64_t kMg1Exact = 1ull << 53;

struct HTree {
  HQueue* q; HNode* nd; uint64_t min_proc; bool analytical;

  __device__ __forceinline__ uint64_t mg1_delay() const { return mg1_queue_delay(q->n, q->newest, q->sig_sq, q->sig); }
  // ---- sorted interval array nd[0..size) (history_tree and history_list) ----
  __device__ __forceinline__ void l_erase(uint32_t i)
  {
    for (uint32_t j = i + 1; j < q->size; ++j) nd[j - 1] = nd[j];
    q->size--;
  }
  __device__ __forceinline__ void l_insert(uint32_t i, uint64_t a, uint64_t b)   // before position i
  {
    for (uint32_t j = q->size; j > i; --j) nd[j] = nd[j - 1];
    nd[i].first = a; nd[i].second = b;
    q->size++;
  }
  // ---- history_tree: circular sorted list.  The header words live in
  // registers for the request (the queue may sit in LDS or HBM; stores to
  // the interval slots would otherwise force them to be reloaded) ----
  struct TL {
    HNode* nd; uint32_t head, cap, n;
    __device__ __forceinline__ uint32_t ph(uint32_t i) const { const uint32_t j = head + i; return j >= cap ? j - cap : j; }
    __device__ __forceinline__ HNode& iv(uint32_t i) const { return nd[ph(i)]; }
    __device__ __forceinline__ void erase(uint32_t i)
    {
      if (i == 0) { head = ph(1); --n; return; }
      for (uint32_t j = i + 1; j < n; ++j) iv(j - 1) = iv(j);
      --n;
    }
    __device__ __forceinline__ void insert(uint32_t i, uint64_t a, uint64_t b)     // before position i (n < cap)
    {
      for (uint32_t j = n; j > i; --j) iv(j) = iv(j - 1);
      HNode& x = iv(i);
      x.first = a; x.second = b;
      ++n;
    }
    // first fit (searchTree, see above): the last interval starting at or
    // before t if it holds [t, t+p], else the first later one of length >= p
    __device__ __forceinline__ int first_fit(uint64_t t, uint64_t p) const
    {
      int lo = 0, hi = (int)n;
      if (n) { const HNode& l = iv(n - 1); if (l.first <= t) { if (t + p <= l.second) return (int)n - 1; lo = (int)n; } }
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (iv(mid).first <= t) lo = mid + 1; else hi = mid; }
      const int j = lo - 1;
      if (j >= 0 && t + p <= iv(j).second) return j;
      for (int i = j + 1; i < (int)n; ++i) { const HNode& x = iv(i); if (x.second - x.first >= p) return i; }
      return -1;
    }
  };
  __device__ __forceinline__ uint64_t tree_delay(uint64_t t, uint64_t p, uint32_t* err)   // computeQueueDelay (:44-126)
  {
    TL L{nd, q->head, q->max_size, q->size};
    uint64_t qd = 0;
    if (L.n >= L.cap) L.erase(0);                              // prune the min node (:52-56)
    const HNode x0 = L.iv(0);
    if (analytical && x0.first > (t + p)) {
      q->analytical++;
      qd = mg1_delay();
    } else {
      const int i = L.first_fit(t, p);
      if (i < 0) { atomicOr(err, GG_DERR_STATE); }
      else {
        HNode& x = L.iv((uint32_t)i);
        const uint64_t a = x.first, b = x.second;
        if (t >= a) {
          if ((t - a) >= min_proc) {
            if ((b - (t + p)) >= min_proc) L.insert((uint32_t)i + 1, t + p, b);
            L.iv((uint32_t)i).second = t;
          } else if ((b - (t + p)) >= min_proc) {
            x.first = t + p;
          } else {
            L.erase((uint32_t)i);
          }
        } else {
          qd = a - t;
          if ((b - (a + p)) >= min_proc) x.first = a + p;
          else L.erase((uint32_t)i);
        }
      }
    }
    q->head = L.head; q->size = L.n;
    return qd;
  }
  // ---- history_tree on a whole wave (every lane, identical arguments; the
  // image in LDS, max_size <= 128): logical interval i in lane i & 63, slot
  // i >> 6.  The same request as tree_delay: the search is two ballots, an
  // insert / erase a shift of the lanes' registers, the write back one
  // store round of the slots that changed (same circular layout) ----
  __device__ __forceinline__ static uint64_t sh64(uint64_t v, uint32_t src) { return (uint64_t)__shfl((long long)v, (int)src); }
  __device__ __forceinline__ static uint64_t rl64(uint64_t v, uint32_t l)
  {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), (int)l) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  }
  __device__ __forceinline__ uint64_t tree_delay_wave(uint64_t t, uint64_t p, uint32_t* err, uint32_t ln)
  {
    const uint32_t cap = q->max_size;
    uint32_t head = q->head, n = q->size;
    if (n >= cap) { head = head + 1 == cap ? 0u : head + 1; --n; }    // prune the min node (:52-56)
    auto phys = [&](uint32_t i) { uint32_t j = head + i; if (j >= cap) j -= cap; if (j >= cap) j -= cap; return j; };
    {
      // the last interval is always [x, UINT64_MAX) (the initial node's end; a
      // request only cuts finite pieces).  A request at t >= x is served there
      // with no delay, and interval 0 starts at or before x, so the M/G/1
      // branch cannot be taken: O(1) on uniform values
      const uint32_t pl = phys(n - 1);
      const HNode last = nd[pl];
      if (last.first <= t) {
        if (t - last.first >= min_proc) {
          nd[pl].second = t;
          nd[phys(n)] = HNode{t + p, last.second};
          ++n;
        } else {
          nd[pl].first = t + p;
        }
        q->head = head; q->size = n;
        wave_sync();
        return 0;
      }
    }
    const bool two = cap > 64;
    uint64_t a0 = 0, b0 = 0, a1 = 0, b1 = 0;
    if (ln < n) { const HNode x = nd[phys(ln)]; a0 = x.first; b0 = x.second; }
    if (two && ln + 64 < n) { const HNode x = nd[phys(ln + 64)]; a1 = x.first; b1 = x.second; }
    uint64_t qd = 0;
    uint32_t ch = n, nn = n;                       // first logical slot that changed, new size
    if (analytical && rl64(a0, 0) > t + p) {
      q->analytical++;
      qd = mg1_delay();
    } else {
      // first fit: j = the last interval starting at or before t
      const bool v0 = ln < n, v1 = ln + 64 < n;
      const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(v0 && a0 <= t)) +
                           (uint32_t)__builtin_popcountll(__ballot(v1 && a1 <= t));
      int i = -1;
      if (cnt > 0) {
        const uint32_t j = cnt - 1;
        const uint64_t bj = j < 64 ? rl64(b0, j) : rl64(b1, j - 64);
        if (t + p <= bj) i = (int)j;
      }
      if (i < 0) {
        const uint64_t m0 = __ballot(v0 && ln >= cnt && b0 - a0 >= p);
        const uint64_t m1 = __ballot(v1 && ln + 64 >= cnt && b1 - a1 >= p);
        i = m0 ? (int)__builtin_ctzll(m0) : (m1 ? 64 + (int)__builtin_ctzll(m1) : -1);
      }
      if (i < 0) {
        if (ln == 0) atomicOr(err, GG_DERR_STATE);
      } else {
        const uint32_t ui = (uint32_t)i;
        const uint64_t a = ui < 64 ? rl64(a0, ui) : rl64(a1, ui - 64);
        const uint64_t b = ui < 64 ? rl64(b0, ui) : rl64(b1, ui - 64);
        uint64_t na = a, nb = b;                    // new interval ui (if it stays)
        int op = 0;                                 // 0 modify, 1 insert (t + p, b) after ui, 2 erase ui
        if (t >= a) {
          if ((t - a) >= min_proc) { nb = t; if ((b - (t + p)) >= min_proc) op = 1; }
          else if ((b - (t + p)) >= min_proc) na = t + p;
          else op = 2;
        } else {
          qd = a - t;
          if ((b - (a + p)) >= min_proc) na = a + p; else op = 2;
        }
        ch = ui;
        if (op == 1) {                              // new(k) = old(k - 1) for k > ui + 1
          const uint32_t s = (ln + 63) & 63;
          const uint64_t pa0 = sh64(a0, s), pb0 = sh64(b0, s), pa1 = sh64(a1, s), pb1 = sh64(b1, s);
          if (ln > ui + 1) { a0 = pa0; b0 = pb0; }
          if (ln + 64 > ui + 1) { a1 = ln == 0 ? pa0 : pa1; b1 = ln == 0 ? pb0 : pb1; }
          const uint32_t k = ui + 1;
          if ((k & 63) == ln) { if (k < 64) { a0 = t + p; b0 = b; } else { a1 = t + p; b1 = b; } }
          nn = n + 1;
        } else if (op == 2) {                       // new(k) = old(k + 1) for k >= ui
          const uint32_t s = (ln + 1) & 63;
          const uint64_t na0 = sh64(a0, s), nb0 = sh64(b0, s), na1 = sh64(a1, s), nb1 = sh64(b1, s);
          if (ln >= ui) { a0 = ln == 63 ? na1 : na0; b0 = ln == 63 ? nb1 : nb0; }
          if (ln + 64 >= ui) { a1 = na1; b1 = nb1; }
          nn = n - 1;
        }
        if (op != 2 && (ui & 63) == ln) { if (ui < 64) { a0 = na; b0 = nb; } else { a1 = na; b1 = nb; } }
      }
    }
    if (ln >= ch && ln < nn) nd[phys(ln)] = HNode{a0, b0};
    if (two && ln + 64 >= ch && ln + 64 < nn) nd[phys(ln + 64)] = HNode{a1, b1};
    q->head = head; q->size = nn;
    wave_sync();
    return qd;
  }
  // replace interval i by up to two intervals (in list order).  The list may
  // overgrow by one only here, and then loses its front (the size check after
  // the scan, queue_model_history_list.cc:128-131): done in place.
  __device__ __forceinline__ void l_replace(uint32_t i, bool k1, uint64_t a1, uint64_t b1, bool k2, uint64_t a2, uint64_t b2)
  {
    if (k1 && !k2) { nd[i].first = a1; nd[i].second = b1; return; }
    if (!k1 && k2) { nd[i].first = a2; nd[i].second = b2; return; }
    if (!k1) { l_erase(i); return; }
    if (q->size < q->max_size) {
      for (uint32_t j = q->size; j > i + 1; --j) nd[j] = nd[j - 1];
      nd[i].first = a1; nd[i].second = b1; nd[i + 1].first = a2; nd[i + 1].second = b2;
      q->size++;
    } else if (i == 0) {                        // the first new interval is the front that goes
      nd[0].first = a2; nd[0].second = b2;
    } else {                                    // drop the front: [1, i) moves down by one
      for (uint32_t j = 1; j < i; ++j) nd[j - 1] = nd[j];
      nd[i - 1].first = a1; nd[i - 1].second = b1; nd[i].first = a2; nd[i].second = b2;
    }
  }
  __device__ __forceinline__ uint64_t list_scan(uint64_t t, uint64_t p)       // computeUsingHistoryList
  {
    uint64_t qd = 0;
    const bool inter = q->aux == 0;
    uint32_t i = 0;
    while (i < q->size) {
      const uint64_t a = nd[i].first, b = nd[i].second;
      if (t >= a && t + p <= b) {
        l_replace(i, t - a >= min_proc, a, t, b - (t + p) >= min_proc, t + p, b);
        return qd;
      }
      if (t < a && a + p <= b) {
        qd += a - t;
        l_replace(i, false, 0, 0, b - (a + p) >= min_proc, a + p, b);
        return qd;
      }
      if (inter && t >= a && t < b) {           // pkt_time moves to b, processing_time -= 0 (as the reference)
        if (t - a >= min_proc) { nd[i].second = t; ++i; } else l_erase(i);
        t = b;
      } else if (inter && t < a) {
        l_erase(i);
        qd += a - t;
        p -= b - a;
        t = b;
      } else {
        ++i;
      }
    }
    return qd;
  }
  // ---- basic: MovingAverage<UInt64>::compute over the window words ----
  __device__ __forceinline__ uint64_t mavg(uint64_t x)
  {
    uint64_t* w = reinterpret_cast<uint64_t*>(nd);
    const uint32_t W = hq_window(q->aux), M = W + 1, avg = q->aux >> 16;
    const uint32_t cws = q->back >= q->front ? q->back - q->front : q->back + M - q->front;
    if (avg != GG_MAVG_MEDIAN) {
      if (cws == W) q->mean += (((double)x / cws) - ((double)w[q->front] / cws));
      else q->mean = (q->mean * cws + (double)x) / (double)(cws + 1);
    }
    w[q->back] = x;                             // addToWindow
    q->back = (q->back + 1) % M;
    if (q->back == q->front) q->front = (q->front + 1) % M;
    if (avg == GG_MAVG_MEDIAN) {
      const uint32_t c2 = q->back >= q->front ? q->back - q->front : q->back + M - q->front;
      return w[(q->front + (c2 / 2) % M) % M];
    }
    return (uint64_t)q->mean;
  }
  __device__ __forceinline__ uint64_t basic_delay(uint64_t t, uint64_t p)
  {
    const uint64_t ref = ((q->aux >> 16) == GG_MAVG_NONE) ? t : mavg(t);
    const uint64_t qd = q->qtime > ref ? q->qtime - ref : 0;
    q->qtime = (q->qtime > ref ? q->qtime : ref) + p;
    q->util += p;
    { uint64_t x = ref + qd + p; if (x > q->last_req) q->last_req = x; }
    q->total_req++;
    return qd;
  }

  __device__ __forceinline__ uint64_t delay(uint64_t t, uint64_t p, uint32_t* err)   // computeQueueDelay
  {
    if (q->type == GG_QM_BASIC) return basic_delay(t, p);
    uint64_t qd;
    if (q->type == GG_QM_HISTORY_LIST) {
      if (analytical && (t + p) < nd[0].first) { q->analytical++; qd = mg1_delay(); }
      else qd = list_scan(t, p);
    } else {
      qd = tree_delay(t, p, err);
    }
    mg1_update(t, p, qd, err);
    return qd;
  }
  // computeQueueDelay on a whole wave (every lane, identical arguments, the
  // queue image in LDS): history_tree lane-parallel, the others as delay()
  __device__ __forceinline__ uint64_t delay_w(uint64_t t, uint64_t p, uint32_t* err, uint32_t ln)
  {
    if (q->type != GG_QM_HISTORY_TREE || q->max_size > 128) return delay(t, p, err);
    const uint64_t qd = tree_delay_wave(t, p, err, ln);
    mg1_update(t, p, qd, err);
    return qd;
  }
  __device__ __forceinline__ void mg1_update(uint64_t t, uint64_t p, uint64_t qd, uint32_t* err)
  {
    const uint64_t ss = q->sig_sq, sg = q->sig;
    const uint64_t nn = q->n, nw = q->newest, ut = q->util, lr = q->last_req, tr = q->total_req;
    const uint64_t x = t + qd + p;
    const uint64_t ss2 = ss + p * p;
    if (ss2 >= kMg1Exact || p >= (1ull << 26)) atomicOr(err, GG_DERR_RANGE);
    q->sig_sq = ss2;                                             // QueueModelMG1::updateQueue
    q->sig = sg + p;
    q->n = nn + 1;
    q->newest = x > nw ? x : nw;
    q->util = ut + p;                                            // updateQueueUtilizationCounters
    q->last_req = x > lr ? x : lr;
    q->total_req = tr + 1;
  }

};

// ---------------------------------------------------------------------------
// One history-tree queue held in a wave's registers for a batch of requests
// (every lane calls every method with identical arguments).  The 128 register
// positions (position x = lane x & 63 of slot x >> 6; 128 = max_size bound)
// form a ring: logical interval i sits at position (hd + i) & 127, hd a
// uniform scalar, so pruning the oldest interval of a full list is hd + 1 and
// moves no lane.  The queue's state costs no memory round trip per request:
// the search is two ballots over the ring range [hd, hd + sz), an insert /
// erase a one-position rotate of both slots (DPP wave_ror / wave_rol, lane 0 /
// 63 taking the other slot's value) masked by the lanes' logical index, the
// header and M/G/1 sums are uniform registers.  load / store move the image
// (HQueue + circular node list, any head) in one round each: load brings the
// list into logical order (hd = 0), store writes it back in logical order
// with head 0.  Same request as HTree::tree_delay + mg1_update (the in-order
// request, t at or after the start of the last interval [x, UINT64_MAX), is
// the O(1) first branch).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t rl64(uint64_t v, uint32_t l)
{
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), (int)l) << 32) |
         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
}
// a wave-uniform 64-bit value into SGPRs (values computed on the vector ALU,
// e.g. FP64, or loaded by an atomic, are otherwise kept in VGPRs)
__device__ __forceinline__ uint64_t rfl64(uint64_t v)
{
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}
// v shifted by SHIFT (a wave shift: one lane has no source) over w rotated by
// ROT (every lane has one), so the lane without a source takes w's
template <int SHIFT, int ROT> __device__ __forceinline__ uint32_t dpp32(uint32_t v, uint32_t w)
{
  const int r = __builtin_amdgcn_mov_dpp((int)w, ROT, 0xf, 0xf, false);
  return (uint32_t)__builtin_amdgcn_update_dpp(r, (int)v, SHIFT, 0xf, 0xf, false);
}
template <int SHIFT, int ROT> __device__ __forceinline__ uint64_t dpp64(uint64_t v, uint64_t w)
{
  return ((uint64_t)dpp32<SHIFT, ROT>((uint32_t)(v >> 32), (uint32_t)(w >> 32)) << 32) | dpp32<SHIFT, ROT>((uint32_t)v, (uint32_t)w);
}
constexpr int kDppWaveShl1 = 0x130;    // lane l <- lane l + 1, lane 63 keeps `old`
constexpr int kDppWaveRol1 = 0x134;    // lane l <- lane (l + 1) & 63
constexpr int kDppWaveShr1 = 0x138;    // lane l <- lane l - 1, lane 0 keeps `old`
constexpr int kDppWaveRor1 = 0x13C;    // lane l <- lane (l - 1) & 63

// lane mask of a 64-bit comparison (one v_cmp into an SGPR pair, no bool
// materialization between compare and ballot)
template <int PRED> __device__ __forceinline__ uint64_t cmp64(uint64_t a, uint64_t b)
{
  return __builtin_amdgcn_uicmpl(a, b, PRED);
}
template <int PRED> __device__ __forceinline__ uint64_t cmp32(uint32_t a, uint32_t b)
{
  return __builtin_amdgcn_uicmp(a, b, PRED);
}
constexpr int kCmpULE = 37, kCmpULT = 36, kCmpUGE = 35, kCmpUGT = 34;     // ICmpInst predicates
__device__ __forceinline__ uint64_t low_lanes(uint32_t n) { return n >= 64 ? ~0ull : ((1ull << n) - 1); }

struct RegQueue {
  uint64_t a0, b0, a1, b1;             // this lane's intervals of slot 0 / slot 1
  uint32_t sz, cap, ln;
  uint32_t hd = 0;                     // position of logical interval 0 (uniform)
  uint64_t sig_sq, sig, nreq, newest, util, last_req, total_req, anl;
  uint64_t min_proc;
  bool analytical;
  uint32_t n_fast = 0, n_anl = 0, n_gen = 0;   // requests by branch (diagnostics)
  uint32_t errs = 0;                   // GG_DERR_* of the batch, reported by store()
  uint32_t* errp = nullptr;

  __device__ __forceinline__ void load(const HQueue* q, const HNode* nd, uint64_t mp, bool an, uint32_t lane)
  {
    // the header is wave-uniform: into SGPRs (a load from memory the kernel
    // also writes lands in VGPRs, and the size would then steer every request
    // through exec-masked branches)
    ln = lane; min_proc = mp; analytical = an; errs = 0; errp = nullptr; hd = 0;
    sz = (uint32_t)__builtin_amdgcn_readfirstlane((int)q->size);
    cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)q->max_size);
    const uint32_t head = (uint32_t)__builtin_amdgcn_readfirstlane((int)q->head);
    sig_sq = rfl64(q->sig_sq); sig = rfl64(q->sig); nreq = rfl64(q->n); newest = rfl64(q->newest);
    util = rfl64(q->util); last_req = rfl64(q->last_req); total_req = rfl64(q->total_req); anl = rfl64(q->analytical);
    a0 = b0 = a1 = b1 = 0;
    uint32_t j = head + ln; if (j >= cap) j -= cap;
    if (ln < sz) { const HNode x = nd[j]; a0 = x.first; b0 = x.second; }
    j = head + ln + 64; if (j >= cap) j -= cap; if (j >= cap) j -= cap;
    if (ln + 64 < sz) { const HNode x = nd[j]; a1 = x.first; b1 = x.second; }
  }
  // load() with the node loads issued beside the header's instead of behind
  // it: every store() writes the list back from slot 0 (head 0), so a queue
  // only ever served through RegQueue (hq_init starts at head 0) has head 0 at
  // every load, and nodes [0, max_size) are the list in order.  The header is
  // checked when it arrives: a queue another form left at head != 0 takes the
  // dependent load().  One memory round trip instead of two.
  __device__ __forceinline__ void load_h0(const HQueue* q, const HNode* nd, uint32_t max_size, uint64_t mp, bool an,
                                          uint32_t lane)
  {
    HNode x0{0, 0}, x1{0, 0};
    if (lane < max_size) x0 = nd[lane];
    if (lane + 64 < max_size) x1 = nd[lane + 64];
    const uint32_t h = (uint32_t)__builtin_amdgcn_readfirstlane((int)q->head);
    if (h != 0) { load(q, nd, mp, an, lane); return; }
    ln = lane; min_proc = mp; analytical = an; errs = 0; errp = nullptr; hd = 0;
    sz = (uint32_t)__builtin_amdgcn_readfirstlane((int)q->size);
    cap = (uint32_t)__builtin_amdgcn_readfirstlane((int)q->max_size);
    sig_sq = rfl64(q->sig_sq); sig = rfl64(q->sig); nreq = rfl64(q->n); newest = rfl64(q->newest);
    util = rfl64(q->util); last_req = rfl64(q->last_req); total_req = rfl64(q->total_req); anl = rfl64(q->analytical);
    const bool v0 = ln < sz, v1 = ln + 64 < sz;
    a0 = v0 ? x0.first : 0; b0 = v0 ? x0.second : 0;
    a1 = v1 ? x1.first : 0; b1 = v1 ? x1.second : 0;
  }
  // load_h0 in two halves, so that a wave can issue other loads while the
  // queue's are in flight: issue() starts the loads into registers and waits
  // for nothing (the header spread over lanes, one 16-B chunk per lane k <
  // sizeof(HQueue) / 16; the nodes as load_h0 reads them); finish() reads
  // the header's fields out of the lanes, which waits for them, and takes
  // the dependent load() when the list does not start at node 0.
  struct Raw { uint4 hc; HNode x0, x1; };
  __device__ __forceinline__ static Raw issue(const HQueue* q, const HNode* nd, uint32_t max_size, uint32_t lane)
  {
    Raw r;
    r.x0 = HNode{0, 0}; r.x1 = HNode{0, 0}; r.hc = make_uint4(0, 0, 0, 0);
    if (lane < max_size) r.x0 = nd[lane];
    if (lane + 64 < max_size) r.x1 = nd[lane + 64];
    if (lane < sizeof(HQueue) / 16) r.hc = reinterpret_cast<const uint4*>(q)[lane];
    return r;
  }
  template <size_t OFF>
  __device__ __forceinline__ static uint32_t hw32(const uint4& c)
  {
    static_assert(OFF % 4 == 0 && OFF < sizeof(HQueue), "a 32-bit header word");
    constexpr uint32_t w = OFF / 4, k = w & 3u;
    const uint32_t v = k == 0 ? c.x : k == 1 ? c.y : k == 2 ? c.z : c.w;
    return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)(w >> 2));
  }
  template <size_t OFF>
  __device__ __forceinline__ static uint64_t hw64(const uint4& c)
  {
    return ((uint64_t)hw32<OFF + 4>(c) << 32) | hw32<OFF>(c);
  }
  __device__ __forceinline__ void finish(const Raw& r, const HQueue* q, const HNode* nd, uint64_t mp, bool an, uint32_t lane)
  {
    const uint32_t h = hw32<offsetof(HQueue, head)>(r.hc);
    if (h != 0) { load(q, nd, mp, an, lane); return; }
    ln = lane; min_proc = mp; analytical = an; errs = 0; errp = nullptr; hd = 0;
    sz = hw32<offsetof(HQueue, size)>(r.hc);
    cap = hw32<offsetof(HQueue, max_size)>(r.hc);
    sig_sq = hw64<offsetof(HQueue, sig_sq)>(r.hc); sig = hw64<offsetof(HQueue, sig)>(r.hc);
    nreq = hw64<offsetof(HQueue, n)>(r.hc); newest = hw64<offsetof(HQueue, newest)>(r.hc);
    util = hw64<offsetof(HQueue, util)>(r.hc); last_req = hw64<offsetof(HQueue, last_req)>(r.hc);
    total_req = hw64<offsetof(HQueue, total_req)>(r.hc); anl = hw64<offsetof(HQueue, analytical)>(r.hc);
    const bool v0 = ln < sz, v1 = ln + 64 < sz;
    a0 = v0 ? r.x0.first : 0; b0 = v0 ? r.x0.second : 0;
    a1 = v1 ? r.x1.first : 0; b1 = v1 ? r.x1.second : 0;
  }
  // Deferred accounting (the pipelined walker): the eight sums stay what
  // load() / finish() read — base values, invariant in the loop around the
  // requests — and the loop carries what its requests add to them: five
  // wave-uniform values for eight (sig and util take the same sum of p, n and
  // total_req the same count, newest and last_req the same maximum), updated
  // with scalar adds and one scalar maximum.  store() writes base + delta;
  // integer adds and maxima are associative, so the header is what account()
  // after every request leaves.  por (every p or-ed) is for the range flag.
  struct Delta {                       // (an aggregate: Delta{} is all zero)
    uint64_t n, p, p2, mx, anl, por;
    __device__ __forceinline__ void add(uint64_t t, uint64_t pp, uint64_t qd)
    {
      ++n; p += pp; p2 += pp * pp; por |= pp;
      const uint64_t x = t + qd + pp;
      mx = x > mx ? x : mx;
    }
  };
  __device__ __forceinline__ void store(HQueue* q, HNode* nd) const { store(q, nd, Delta{}); }
  __device__ __forceinline__ void store(HQueue* q, HNode* nd, const Delta& d) const
  {
    uint32_t e = errs;
    const uint64_t ss = sig_sq + d.p2;
    // account()'s range check once for the batch: sig_sq only grows, so the
    // last value tells whether any was out of range, and some p had a bit at
    // or above 2^26 iff their or has
    if (d.n && (ss >= kMg1Exact || (d.por >> 26))) e |= GG_DERR_RANGE;
    if (e && errp && ln == 0) atomicOr(errp, e);
    const uint32_t l0 = li(), l1 = l0 ^ 64u;
    if (l0 < sz) nd[l0] = HNode{a0, b0};
    if (l1 < sz) nd[l1] = HNode{a1, b1};
    q->size = sz; q->head = 0;
    q->sig_sq = ss; q->sig = sig + d.p; q->n = nreq + d.n; q->newest = d.mx > newest ? d.mx : newest;
    q->util = util + d.p; q->last_req = d.mx > last_req ? d.mx : last_req; q->total_req = total_req + d.n;
    q->analytical = anl + d.anl;
  }
  // this lane's logical index in slot 0 (slot 1: the same ^ 64), and the
  // position of logical interval i
  __device__ __forceinline__ uint32_t li() const { return (ln - hd) & 127u; }
  __device__ __forceinline__ uint32_t pos(uint32_t i) const { return (hd + i) & 127u; }
  // the bounds at position x: both slots read, then a scalar select (no branch)
  __device__ __forceinline__ uint64_t PA(uint32_t x) const
  {
    const uint32_t l = x & 63; const uint64_t u = rl64(a0, l), v = rl64(a1, l); return x < 64 ? u : v;
  }
  __device__ __forceinline__ uint64_t PB(uint32_t x) const
  {
    const uint32_t l = x & 63; const uint64_t u = rl64(b0, l), v = rl64(b1, l); return x < 64 ? u : v;
  }
  // logical interval i's bounds
  __device__ __forceinline__ uint64_t A(uint32_t i) const { return PA(pos(i)); }
  __device__ __forceinline__ uint64_t B(uint32_t i) const { return PB(pos(i)); }
  __device__ __forceinline__ void set(uint32_t i, uint64_t a, uint64_t b)
  {
    const uint32_t x = pos(i);
    if ((x & 63) == ln) { if (x < 64) { a0 = a; b0 = b; } else { a1 = a; b1 = b; } }
  }
  // One-position rotates over the 128 positions, masked by the lanes' logical
  // index.  The wave shift leaves the lane without a source (0 going up, 63
  // going down) at the `old` operand, which is the other slot rotated: that
  // lane so takes the other slot's end, which carries slot 0 lane 63 <-> slot 1
  // lane 0 and closes the ring, slot 1 lane 63 <-> slot 0 lane 0.
  // up: new[i] = old[i - 1] for logical i with m0 / m1 set (slot 0 / 1)
  __device__ __forceinline__ void rotate_up(bool m0, bool m1)
  {
    const uint64_t pa0 = dpp64<kDppWaveShr1, kDppWaveRor1>(a0, a1), pa1 = dpp64<kDppWaveShr1, kDppWaveRor1>(a1, a0);
    a0 = m0 ? pa0 : a0; a1 = m1 ? pa1 : a1;
    __builtin_amdgcn_sched_barrier(0);               // starts, then ends: four temporaries live, not eight
    const uint64_t pb0 = dpp64<kDppWaveShr1, kDppWaveRor1>(b0, b1), pb1 = dpp64<kDppWaveShr1, kDppWaveRor1>(b1, b0);
    b0 = m0 ? pb0 : b0; b1 = m1 ? pb1 : b1;
  }
  // down: new[i] = old[i + 1]
  __device__ __forceinline__ void rotate_down(bool m0, bool m1)
  {
    const uint64_t na0 = dpp64<kDppWaveShl1, kDppWaveRol1>(a0, a1), nb0 = dpp64<kDppWaveShl1, kDppWaveRol1>(b0, b1);
    const uint64_t na1 = dpp64<kDppWaveShl1, kDppWaveRol1>(a1, a0), nb1 = dpp64<kDppWaveShl1, kDppWaveRol1>(b1, b0);
    a0 = m0 ? na0 : a0; b0 = m0 ? nb0 : b0;
    a1 = m1 ? na1 : a1; b1 = m1 ? nb1 : b1;
  }
  // new[i] = old[i - 1] for i > k (logical 127, beyond any list here, is lost)
  __device__ __forceinline__ void shift_up(uint32_t k) { const uint32_t l = li(); rotate_up(l > k, (l ^ 64u) > k); }
  // new[i] = old[i + 1] for i >= k (logical 127 takes what was logical 0's position: not an interval)
  __device__ __forceinline__ void shift_down(uint32_t k) { const uint32_t l = li(); rotate_down(l >= k, (l ^ 64u) >= k); }
  // QueueModelMG1::updateQueue + updateQueueUtilizationCounters.  RB: the
  // sums are read back into SGPRs (readfirstlane; they are uniform).  That
  // pays where the loop around the request carries them in SGPRs (the step
  // kernel's port batches: -1.5 % of k_c_step with it, +0.9 % without); the
  // pipelined walker's loop joins branches on values loaded from memory and
  // holds the sums in VGPRs whatever is done here, so a read-back there is 16
  // readfirstlane and as many copies back a serve (-2.9 % of k_c_walk
  // without it; profiles/r15) — that loop now carries a Delta instead and
  // never comes here.  The NoC batches choose at their call sites
  // (request<TAIL, RB>; profiles/r19).
  template <bool RB> __device__ __forceinline__ static uint64_t rd64(uint64_t v) { return RB ? rfl64(v) : v; }
  template <bool RB> __device__ __forceinline__ void account(uint64_t t, uint64_t p, uint64_t qd)
  {
    sig_sq = rd64<RB>(sig_sq + p * p);                               // QueueModelMG1::updateQueue
    sig = rd64<RB>(sig + p);
    if (sig_sq >= kMg1Exact || p >= (1ull << 26)) errs |= GG_DERR_RANGE;
    nreq = rd64<RB>(nreq + 1);
    const uint64_t x = t + qd + p;
    newest = rd64<RB>(x > newest ? x : newest);
    util = rd64<RB>(util + p);                                       // updateQueueUtilizationCounters
    last_req = rd64<RB>(x > last_req ? x : last_req);
    total_req = rd64<RB>(total_req + 1);
    anl = rd64<RB>(anl);
  }
  // The request in halves, for a pipeline stage that forwards its packet
  // as soon as the delay is known and does the bookkeeping while the next
  // stage runs (this queue's next request comes from the same wave, after
  // it).  prune() is what every request does first: a full list drops its
  // oldest interval (the min node, :52-56), which in the ring is the head
  // moving one position; search() only reads the queue and gives the delay
  // and the (logical) interval that serves [t, t+p]; apply() updates the
  // interval list and the M/G/1 sums with that result.  Nothing touches the
  // queue between the halves, so prune, search ... apply is the request made
  // at the time of apply(): a wave that knows its next request ahead of the
  // packet's arrival runs prune() and search() while it waits.
  // One vector search serves every case (the last interval [x, inf) is found
  // by the same compares): the interval holding t fits [t, t+p] -> no delay,
  // known after two compares; otherwise either the analytical branch
  // (interval 0 starts after t + p; never with a fit, whose interval starts at
  // or before t) or the first later interval long enough, which is the least
  // logical index of its mask: the 128-bit mask rotated right by hd.
  // A loop around the requests carries sz and hd through joins of branches
  // on values loaded from memory, where the compiler holds them in VGPRs and
  // would steer every use through exec masks: each half reads them back into
  // SGPRs first (they are uniform).
  __device__ __forceinline__ static uint32_t rd32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  __device__ __forceinline__ void uni() { sz = rd32(sz); hd = rd32(hd); }
  enum : uint32_t { kFit = 0, kAnalytical = 1, kLater = 2, kNone = 3 };
  struct Found { uint64_t qd; uint32_t ui, kind; };
  __device__ __forceinline__ void prune()
  {
    uni();
    const bool full = sz >= cap;
    hd = full ? (hd + 1) & 127u : hd;
    sz = full ? sz - 1 : sz;
  }
  // d: what the batch has added to the sums so far under deferred accounting
  // (the analytical branch forms base + delta here; nothing else reads them)
  __device__ __forceinline__ Found search(uint64_t t, uint64_t p, const Delta& d = Delta{}) const
  {
    const uint64_t tp = t + p;
    const uint32_t hd = rd32(this->hd), sz = rd32(this->sz);
    const uint32_t l0 = (ln - hd) & 127u;
    const uint64_t v0 = cmp32<kCmpULT>(l0, sz), v1 = cmp32<kCmpULT>(l0 ^ 64u, sz);   // the ring range [hd, hd + sz)
    const uint64_t le0 = cmp64<kCmpULE>(a0, t) & v0, le1 = cmp64<kCmpULE>(a1, t) & v1;
    const uint64_t f0 = le0 & cmp64<kCmpUGE>(b0, tp), f1 = le1 & cmp64<kCmpUGE>(b1, tp);
    if (f0 | f1) {                                                   // a <= t, t + p <= b: no delay (one lane at most)
      const uint32_t x = f0 ? (uint32_t)__builtin_ctzll(f0) : 64u + (uint32_t)__builtin_ctzll(f1);
      return Found{0ull, (x - hd) & 127u, kFit};
    }
    const uint32_t hs = hd & 63u;
    if (analytical) {                                                // interval 0 (position hd) starts after t + p
      const uint64_t g = hd < 64 ? cmp64<kCmpUGT>(a0, tp) : cmp64<kCmpUGT>(a1, tp);
      if ((g >> hs) & 1ull)
        return Found{rfl64(mg1_queue_delay(nreq + d.n, d.mx > newest ? d.mx : newest, sig_sq + d.p2, sig + d.p)), 0u,
                     kAnalytical};
    }
    const uint64_t m0 = ~le0 & v0 & cmp64<kCmpUGE>(b0 - a0, p);      // the first later interval long enough
    const uint64_t m1 = ~le1 & v1 & cmp64<kCmpUGE>(b1 - a1, p);
    if ((m0 | m1) == 0) return Found{0ull, 0u, kNone};
    const uint64_t x0 = hd < 64 ? m0 : m1, x1 = hd < 64 ? m1 : m0;   // bit i of (r1, r0): logical interval i
    const uint64_t r0 = hs ? (x0 >> hs) | (x1 << (64u - hs)) : x0, r1 = hs ? (x1 >> hs) | (x0 << (64u - hs)) : x1;
    const uint32_t ui = r0 ? (uint32_t)__builtin_ctzll(r0) : 64u + (uint32_t)__builtin_ctzll(r1);
    return Found{A(ui) - t, ui, kLater};
  }
  // The fit whose interval splits in two is three requests in four on a busy
  // port: it runs from here to the updated list with no branch but the
  // dispatch on kind.  Keeping the left part [a, t] and the right part
  // [t+p, b] are scalar conditions.  One rotate (an empty mask unless both
  // are kept) copies interval ui to ui + 1; then a part kept alone changes one
  // bound of ui, and of two parts the left one is ui with end t, the right
  // one ui + 1 with start t+p: two selects on the lanes' logical index, one
  // writing starts and one ends.  A fit that keeps neither part erases the
  // interval behind that.  update() is the interval list's half of apply()
  // (true: the request was analytical, which changes no interval); the sums
  // follow at once (apply(t, p, s); RB: see account()) or as deltas
  // (apply(t, p, s, d)).
  template <bool RB = false> __device__ __forceinline__ void apply(uint64_t t, uint64_t p, const Found& s)
  {
    if (update(t, p, s)) ++anl;
    account<RB>(t, p, s.qd);
  }
  __device__ __forceinline__ void apply(uint64_t t, uint64_t p, const Found& s, Delta& d)
  {
    d.anl += update(t, p, s) ? 1u : 0u;
    d.add(t, p, s.qd);
  }
  __device__ __forceinline__ bool update(uint64_t t, uint64_t p, const Found& s)
  {
    const uint64_t tp = t + p;
    const uint32_t ui = rd32(s.ui), kind = rd32(s.kind);
    uni();
    if (kind == kFit) {
      ++n_gen;
      const uint32_t x = pos(ui);
      const uint64_t ts = rfl64(t), tps = rfl64(tp);
      const bool keepL = ts - PA(x) >= min_proc, keepR = PB(x) - tps >= min_proc, split = keepL && keepR;
      const uint32_t l0 = li(), l1 = l0 ^ 64u;
      const uint32_t k = split ? ui : 127u;
      rotate_up(l0 > k, l1 > k);
      const uint32_t sa = keepL ? 128u : ui, sa1 = split ? ui + 1 : 128u, sb = keepL ? ui : 128u;   // 128: no lane
      a0 = (l0 == sa || l0 == sa1) ? tp : a0; a1 = (l1 == sa || l1 == sa1) ? tp : a1;
      b0 = l0 == sb ? t : b0; b1 = l1 == sb ? t : b1;
      sz += split ? 1u : 0u;
      if (!keepL && !keepR) { shift_down(ui); --sz; }
    } else if (kind == kAnalytical) {
      ++n_anl;
    } else if (kind == kNone) {
      ++n_gen;
      errs |= GG_DERR_STATE;
    } else {
      ++n_gen;
      const uint64_t a = A(ui), b = B(ui);
      if (b - (a + p) >= min_proc) set(ui, a + p, b);
      else { shift_down(ui); --sz; }
    }
    return kind == kAnalytical;
  }
  // computeQueueDelay (queue_model_history_tree.cc:44-126) + QueueModelMG1::updateQueue.
  // The O(1) branch for a request served by the last interval stands in
  // front of the general request, search() + apply().  TAIL: also the O(1)
  // branch for requests served by the last two intervals (in-order streams:
  // SELF / injection ports); the walkers' requests land mid-list 84 % of the
  // time and skip that check (TAIL = false: search + apply serve those
  // requests too, with the same result).  RB: see account(); the caller
  // chooses by what its loop around the requests carries the sums in.
  template <bool TAIL = true, bool RB = true>
  __device__ __forceinline__ uint64_t request(uint64_t t, uint64_t p, uint32_t* err)
  {
    errp = err;
    prune();
    {
      const uint64_t la = A(sz - 1), lb = B(sz - 1);
      if (la <= t && t + p <= lb && lb - (t + p) >= min_proc) {      // the last interval: no search, no delay
        ++n_fast;
        if (t - la >= min_proc) { set(sz - 1, la, t); set(sz, t + p, lb); ++sz; }
        else set(sz - 1, t + p, lb);
        account<RB>(t, p, 0);
        return 0;
      }
      if (TAIL && sz >= 2 && t < la && t >= A(sz - 2)) {
        // the tail: interval sz-2 is the last one starting at or before t (and
        // interval 0 starts before t: no M/G/1).  Either [t, t+p] fits in it, or
        // the first later interval long enough is the last one (unbounded)
        ++n_fast;
        uint64_t qd = 0;
        const uint32_t i2 = sz - 2, i1 = sz - 1;
        const uint64_t a2 = A(i2), b2 = B(i2);
        if (t + p <= b2) {
          if (t - a2 >= min_proc) {
            if (b2 - (t + p) >= min_proc) { set(i1 + 1, la, lb); set(i1, t + p, b2); ++sz; }
            set(i2, a2, t);
          } else if (b2 - (t + p) >= min_proc) {
            set(i2, t + p, b2);
          } else {
            set(i2, la, lb); --sz;                                     // erase interval sz-2
          }
        } else {
          qd = la - t;                                                 // queued behind the busy period
          if (lb - (la + p) >= min_proc) set(i1, la + p, lb);
          else --sz;                                                   // erase the last interval
        }
        account<RB>(t, p, qd);
        return qd;
      }
    }
    const Found s = search(t, p);
    apply<RB>(t, p, s);
    return s.qd;
  }
};

// Latency::toPicosec / Time::toCycles (time_types.h:81-109), double and ceil.
// At 1 GHz (every clock domain of carbon_sim.cfg) both are exact integer
// maps below 2^52 ps: 1000 * cycles / 1.0 is exact, and the correctly
// rounded ps / 1000.0 of a non-multiple of 1000 stays more than 2^-11 away
// from an integer, so its ceil is (ps + 999) / 1000.  Integer arithmetic
// there, the double formula elsewhere.
__device__ __forceinline__ uint64_t lat_to_ps(uint64_t cycles, double f)
{
  if (f == 1.0 && cycles < (1ull << 42)) return 1000 * cycles;
  return (uint64_t)ceil(((double)1000 * cycles) / f);
}
__device__ __forceinline__ uint64_t time_to_cycles(uint64_t ps, double f)
{
  if (f == 1.0 && ps < (1ull << 52)) return (ps + 999) / 1000;
  return (uint64_t)ceil(((double)ps * f) / 1.0e3);
}

struct NocParams {
  uint32_t tiles, w, h, flit_width, router_delay, link_delay, qm, analytical, max_size, net_model;
  uint32_t qtype, qaux;                 // router queue model (GG_QM_*) and its hq_aux parameter
  double f;
};

__device__ __forceinline__ uint64_t nflits(const NocParams& P, uint32_t bits)
{
  return (bits % P.flit_width == 0) ? bits / P.flit_width : bits / P.flit_width + 1;   // computeNumFlits
}

__device__ __forceinline__ void cadd(uint64_t* c, uint32_t tile, int k, uint64_t v)
{
  if (v) atomicAdd((unsigned long long*)&c[(uint64_t)tile * GG_NUM_NET_COUNTERS + k], (unsigned long long)v);
}


// emesh_hop_counter (network_model_emesh_hop_counter.cc:143-157) / magic
// (network_model_magic.cc:5-21) for one packet, with the sender / receiver
// counters and processReceivedPacket's serialization (network_model.cc:142-150).
// Returns the time the packet is handed to the receiver; zl = zero-load part.
__device__ __forceinline__ uint64_t route_closed_form(const NocParams& P, uint32_t s, uint32_t d, uint32_t bits,
                                                      uint64_t t, uint64_t& zl, uint64_t* ctr)
{
  zl = 0;
  if (s == d) return t;                           // processCornerCases: self-sends cost nothing
  if (P.net_model == GG_NET_MAGIC) {
    cadd(ctr, s, GG_NC_PACKETS_SENT, 1); cadd(ctr, s, GG_NC_BITS_SENT, bits);
    const uint64_t l = lat_to_ps(1, P.f);
    t += l; zl += l;
    cadd(ctr, d, GG_NC_PACKETS_RECEIVED, 1); cadd(ctr, d, GG_NC_BITS_RECEIVED, bits);
    cadd(ctr, d, GG_NC_TOTAL_LATENCY_PS, zl);
    return t;
  }
  const uint64_t nf = nflits(P, bits);
  cadd(ctr, s, GG_NC_PACKETS_SENT, 1); cadd(ctr, s, GG_NC_FLITS_SENT, nf); cadd(ctr, s, GG_NC_BITS_SENT, bits);
  const int sx = (int)(s % P.w), sy = (int)(s / P.w), dx = (int)(d % P.w), dy = (int)(d / P.w);
  const uint64_t hops = (uint64_t)(abs(sx - dx) + abs(sy - dy));
  const uint64_t lat = lat_to_ps(hops * ((uint64_t)P.router_delay + P.link_delay), P.f);
  t += lat; zl += lat;
  cadd(ctr, s, GG_NC_BUFFER_WRITES, nf * hops); cadd(ctr, s, GG_NC_BUFFER_READS, nf * hops);
  cadd(ctr, s, GG_NC_SWITCH_ALLOC, hops); cadd(ctr, s, GG_NC_CROSSBAR, nf * hops);
  cadd(ctr, s, GG_NC_LINK_TRAVERSALS, nf * hops);
  const uint64_t ser = lat_to_ps(nf, P.f);
  t += ser; zl += ser;
  cadd(ctr, d, GG_NC_PACKETS_RECEIVED, 1); cadd(ctr, d, GG_NC_FLITS_RECEIVED, nf);
  cadd(ctr, d, GG_NC_BITS_RECEIVED, bits); cadd(ctr, d, GG_NC_TOTAL_LATENCY_PS, zl);
  return t;
}

}  // namespace gg

// ATAC (gg_noc_atac.hip): its state hangs off the context (gg_ctx::atac)
gg_status gg_atac_alloc(gg_ctx* ctx, const gg_atac_params* p);   // NULL: the defaults
void      gg_atac_free(gg_ctx* ctx);
gg_status gg_atac_reset(gg_ctx* ctx, hipStream_t s);
gg_status gg_atac_run(gg_ctx* ctx, const gg_packets* pk, const gg_packet_out* out, const gg_packet_out* bout,
                      uint64_t nb, hipStream_t s);
// the mesh stage pipeline as ATAC's ENet (gg_noc.hip: noc_hbh_stages), and the
// per-packet time / zero-load / contention arrays it leaves
gg_status gg_noc_enet_stages(gg_ctx* ctx, const uint32_t* src, const uint32_t* dst_inj, const uint32_t* dst_xy,
                             const uint32_t* dst_self, const uint32_t* len, const uint64_t* t0, uint64_t n, hipStream_t s);
void gg_noc_packet_state(gg_ctx* ctx, uint64_t** t, uint64_t** zl, uint64_t** ct);
void gg_noc_set_enet(gg_ctx* ctx, uint32_t router_delay);
// accessors of the NoC state (gg_noc.hip) for the coherent path
gg::NocParams gg_noc_params(gg_ctx* ctx);
uint64_t* gg_noc_ctr(gg_ctx* ctx);
// hop-by-hop stage pipeline over up to `cap` packets (*n_dev of them when given);
// khi / klo: canonical tie-break keys (NULL: the packet index)
gg_status gg_noc_hbh(gg_ctx* ctx, const uint32_t* src, const uint32_t* dst, const uint32_t* len, const uint64_t* t0,
                     const uint64_t* khi, const uint64_t* klo, uint64_t cap, const uint32_t* n_dev, hipStream_t s);
const uint64_t* gg_noc_packet_times(gg_ctx* ctx);   // arrival times of the last pipeline run
// the router queues [tile * 6 + port] (ports 0..4 mesh SELF LEFT RIGHT DOWN UP, 5 injection)
void gg_noc_queues(gg_ctx* ctx, gg::HQueue** q, gg::HNode** nd);
