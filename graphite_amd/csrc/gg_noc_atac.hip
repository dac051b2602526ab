// gg_noc_atac.hip — the ATAC network model (models/network_model_atac.cc) for
// the NoC batch API on MI355X (gfx950).
//
// A packet's queues form a DAG (XY routing inside a cluster, then one way
// through the hubs): injection port -> ENet X chain -> ENet Y chain -> SELF
// port (ENet packets) or the access point's sixth port -> send hub -> receive
// hub + receive net.  Every queue serves its requests in (arrival time,
// packet index) order, the order of one global event queue, so
// the batch runs as stages separated by launches:
//   ENet     the mesh stage pipeline of gg_noc.hip (gg_noc_enet_stages) with a
//            per-packet ENet target: the receiver, or the sender's access
//            point (routePacketOnENet, :370-403; ONet packets are masked out
//            of the SELF stage);
//   k_atac_port<AP>    one wave per access-point tile: the ENet router's sixth
//            output port and its link to the hub (:411-421);
//   k_atac_port<HUB>   one workgroup per cluster (all waves sort, one serves):
//            the send hub's output port and the optical link; a broadcast
//            becomes its per-cluster copy records here (:429-478);
//   k_atac_receive     one workgroup per (cluster, receive net): the receive
//            hub's port of that net and the star router's cluster_size ports
//            see the same requests at the same times (one Hop, :480-539), so
//            one sorted event list feeds a wave per queue; a broadcast asks
//            every star port and takes the largest delay
//            (RouterModel::OUTPUT_PORT_ALL); then the deliveries.
// No stage waits across workgroups: a stage ends with its launch.
#include "gg_dev.h"
#include "gg_noc_stage.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {
using namespace gg;

enum { R_NONE = 0, R_ENET = 1, R_ONET = 2, R_BCAST = 3 };   // a packet's global route (computeGlobalRoute, :797-819)

struct AtacDev {
  NocParams P;                       // the ENet's (router_delay = enet_router_delay, link_delay = 1)
  gg_atac_params A;
  uint32_t C;                        // clusters
  const uint32_t *cluster_of, *ap_of, *hub_of, *star_of, *members;   // members[c * cluster_size + star index] = tile
  // queues: [0, T) the access-point port of a tile | [T, T + C) send hubs |
  // then per (cluster, net) g = c * nets + net: the receive hub's port at
  // rh0 + g and the star router's ports at st0 + g * cluster_size + index
  HQueue* q; HNode* nd;
  uint64_t* ctr;                     // [tile][GG_NUM_NET_COUNTERS] (the NoC state's)
  uint64_t* actr;                    // [tile][GG_NUM_ATAC_COUNTERS]
  uint32_t* err;
  __device__ uint64_t rh0() const { return (uint64_t)P.tiles + C; }
  __device__ uint64_t st0() const { return rh0() + (uint64_t)C * A.num_receive_nets; }
};

struct AtacPk {                      // the batch and its per-packet scratch
  const uint32_t *src, *dst, *len; const uint64_t* t0;
  uint32_t n; uint64_t nb;
  uint8_t* route;                    // R_*
  uint32_t *dinj, *dxy, *dself;      // the ENet stages' destinations
  uint32_t *bidx, *bpkt;             // broadcast ordinal of a packet / packet of a broadcast
  uint32_t* nbc;                     // broadcasts of the batch that have an ordinal (<= nb)
  uint64_t *t, *zl, *ct;             // the mesh stages' packet state (time, zero-load, contention)
  uint64_t *rt, *rzl, *rct;          // records after the send hub: unicast k at k, copy (b, cluster) at n + b * C + cluster
  gg_packet_out out, bout;
};

__device__ __forceinline__ void aadd(uint64_t* c, uint32_t tile, int k, uint64_t v)
{
  if (v) atomicAdd((unsigned long long*)&c[(uint64_t)tile * GG_NUM_ATAC_COUNTERS + k], (unsigned long long)v);
}
__device__ __forceinline__ uint32_t rl32(uint32_t v, uint32_t l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)l); }
__device__ __forceinline__ void gsync()   // global-memory ordering between the lanes of one wave
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// One output-port queue served by a wave: a history tree of <= kQMaxNoc
// intervals lives in the wave's registers (RegQueue); the other queue models
// (and longer lists) go through HTree on the HBM image, one lane.  Every lane
// calls request() with identical arguments and gets the same delay.
struct WaveQueue {
  bool on, reg; uint32_t ln;
  RegQueue rq; HQueue* q; HNode* nd; bool analytical;
  __device__ __forceinline__ void open(const NocParams& P, HQueue* q_, HNode* nd_, uint32_t lane)
  {
    on = P.qm != 0; reg = P.qtype == GG_QM_HISTORY_TREE && P.max_size <= kQMaxNoc;
    q = q_; nd = nd_; ln = lane; analytical = P.analytical != 0;
    if (on && reg) rq.load(q, nd, 1, analytical, ln);
  }
  __device__ __forceinline__ uint64_t request(uint64_t cycles, uint64_t nf, uint32_t* err)
  {
    if (!on) return 0;
    if (reg) return rq.request<true>(cycles, nf, err);
    uint64_t d = 0;
    if (ln == 0) { HTree tr{q, nd, 1, analytical}; d = tr.delay(cycles, nf, err); }
    return rfl64(d);
  }
  __device__ __forceinline__ void close() { if (on && reg) rq.store(q, nd); }
};

// in-place heap sort by one thread (buckets beyond the LDS sort)
__device__ __forceinline__ void serial_sort(SK* a, uint32_t n)
{
  auto sift = [&](uint32_t i, uint32_t m) {
    const SK x = a[i];
    for (;;) {
      uint32_t c = 2 * i + 1;
      if (c >= m) break;
      if (c + 1 < m && sk_lt(a[c], a[c + 1])) ++c;
      if (!sk_lt(x, a[c])) break;
      a[i] = a[c]; i = c;
    }
    a[i] = x;
  };
  for (uint32_t i = n / 2; i-- > 0;) sift(i, n);
  for (uint32_t m = n; m-- > 1;) { const SK x = a[0]; a[0] = a[m]; a[m] = x; sift(0, m); }
}

// The n requests of a wave's bucket sorted by (time, packet index): in the
// wave's LDS (bitonic) up to cap, else in the bucket's HBM scratch (one lane).
template <class Fill>
__device__ SK* wave_sorted(SK* lds, uint32_t cap, SK* hbm, uint32_t n, uint32_t ln, Fill fill)
{
  if (n <= cap) {
    uint32_t M = 1;
    while (M < n) M <<= 1;
    for (uint32_t i = ln; i < M; i += 64) lds[i] = i < n ? fill(i) : SK{~0ull, ~0u, ~0u};
    nsync();
    for (uint32_t kk = 2; kk <= M; kk <<= 1)
      for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
        for (uint32_t i = ln; i < M; i += 64) {
          const uint32_t l = i ^ j;
          if (l > i) {
            const SK x = lds[i], y = lds[l];
            if (((i & kk) == 0) == sk_lt(y, x)) { lds[i] = y; lds[l] = x; }
          }
        }
        nsync();
      }
    return lds;
  }
  for (uint32_t i = ln; i < n; i += 64) hbm[i] = fill(i);
  gsync();
  if (ln == 0) serial_sort(hbm, n);
  gsync();
  return hbm;
}

// The same with every thread of the workgroup (all of them must call it).
template <class Fill>
__device__ SK* block_sorted(SK* lds, uint32_t cap, SK* hbm, uint32_t n, Fill fill)
{
  const uint32_t tid = threadIdx.x;
  if (n <= cap) {
    uint32_t M = 1;
    while (M < n) M <<= 1;
    for (uint32_t i = tid; i < M; i += blockDim.x) lds[i] = i < n ? fill(i) : SK{~0ull, ~0u, ~0u};
    __syncthreads();
    block_bitonic(lds, M, [](const SK& x, const SK& y) { return sk_lt(x, y); });
    return lds;
  }
  for (uint32_t i = tid; i < n; i += blockDim.x) hbm[i] = fill(i);
  __threadfence();
  __syncthreads();
  if (tid == 0) serial_sort(hbm, n);
  __threadfence();
  __syncthreads();
  return hbm;
}

// ---------------------------------------------------------------------------
// batch setup
// ---------------------------------------------------------------------------
// broadcast ordinals in batch order (one workgroup: a chunk per thread)
__global__ __launch_bounds__(1024) void k_atac_bscan(AtacDev D, AtacPk K)
{
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t per = ((uint64_t)K.n + 1023) / 1024;
  const uint32_t b0 = (uint32_t)min((uint64_t)K.n, t * per), b1 = (uint32_t)min((uint64_t)K.n, b0 + per);
  uint32_t c = 0;
  for (uint32_t k = b0; k < b1; ++k) c += K.dst[k] == GG_BROADCAST && K.src[k] < D.P.tiles;
  part[t] = c;
  __syncthreads();
  if (t == 0) {
    uint32_t a = 0;
    for (uint32_t i = 0; i < 1024; ++i) { const uint32_t v = part[i]; part[i] = a; a += v; }
    if (a != K.nb) atomicOr(D.err, K.nb ? GG_DERR_CAP : GG_DERR_RANGE);   // num_broadcasts disagrees / a broadcast in gg_noc_route_batch
    *K.nbc = (uint32_t)min((uint64_t)a, K.nb);
  }
  __syncthreads();
  uint32_t a = part[t];
  for (uint32_t k = b0; k < b1; ++k) {
    const bool b = K.dst[k] == GG_BROADCAST && K.src[k] < D.P.tiles;
    const bool keep = b && a < K.nb;            // never an ordinal beyond the caller's buffers
    K.bidx[k] = keep ? a : ~0u;
    if (keep) K.bpkt[a] = k;
    a += b;
  }
}

// a packet's global route, its ENet stage destinations and the sender's
// broadcast totals (updateSendCounters, network_model.cc:244-250)
__global__ void k_atac_prep(AtacDev D, AtacPk K)
{
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K.n) return;
  const NocParams& P = D.P;
  const uint32_t s = K.src[k], d = K.dst[k];
  uint8_t r = R_NONE;
  uint32_t inj = s < P.tiles ? s : 0u, xy = inj, self = inj;
  if (s >= P.tiles || (d >= P.tiles && d != GG_BROADCAST)) atomicOr(D.err, GG_DERR_RANGE);
  else if (d == GG_BROADCAST) { if (K.bidx[k] != ~0u) r = R_BCAST; }
  else if (s != d) {
    r = R_ONET;
    if (D.cluster_of[s] == D.cluster_of[d]) r = R_ENET;
    else if (D.A.global_routing == GG_ATAC_DISTANCE_BASED) {
      const int sx = (int)(s % P.w), sy = (int)(s / P.w), dx = (int)(d % P.w), dy = (int)(d / P.w);
      if ((uint32_t)(abs(sx - dx) + abs(sy - dy)) <= D.A.unicast_distance_threshold) r = R_ENET;
    }
  }
  if (r == R_ENET) inj = xy = self = d;
  else if (r != R_NONE) { inj = s ^ 1u; xy = D.ap_of[s]; self = s; }   // injected, to the access point, no SELF port
  K.route[k] = r; K.dinj[k] = inj; K.dxy[k] = xy; K.dself[k] = self;
  if (r == R_BCAST) {
    const uint32_t bits = K.len[k];
    cadd(D.ctr, s, GG_NC_PACKETS_BROADCASTED, 1); cadd(D.ctr, s, GG_NC_FLITS_BROADCASTED, nflits(P, bits));
    cadd(D.ctr, s, GG_NC_BITS_BROADCASTED, bits);
  }
}

// bucket keys of the port stages; ~0 = not in the stage
template <int STAGE>   // 0: access-point port (tile), 1: send hub (cluster), 2: receive (cluster * nets + net) over records
__global__ void k_atac_keys(AtacDev D, AtacPk K, uint64_t nrec, uint32_t* keys, uint32_t* counts)
{
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= nrec) return;
  uint32_t key = ~0u;
  if (STAGE < 2) {
    const uint8_t rt = K.route[r];
    if (rt >= R_ONET) key = STAGE == 0 ? K.dxy[r] : D.cluster_of[K.src[r]];
  } else if (r < K.n) {
    if (K.route[r] == R_ONET) key = D.cluster_of[K.dst[r]] * D.A.num_receive_nets + D.cluster_of[K.src[r]] % D.A.num_receive_nets;
  } else {
    const uint64_t b = (r - K.n) / D.C, c = (r - K.n) % D.C;
    if (b < *K.nbc) key = (uint32_t)c * D.A.num_receive_nets + D.cluster_of[K.src[K.bpkt[b]]] % D.A.num_receive_nets;
  }
  keys[r] = key;
  if (key != ~0u) atomicAdd(&counts[key], 1u);
}

// ---------------------------------------------------------------------------
// Port stages: one wave per queue.  Access-point ports: kAWaves queues per
// workgroup, each wave sorting its own requests.  Send hubs (a cluster's whole
// optical traffic in one queue): one per workgroup, all its waves sort, wave 0
// serves.
// ---------------------------------------------------------------------------
constexpr uint32_t kAWaves = 4, kAPk = 2048;
constexpr size_t kALds = (size_t)kAWaves * kAPk * sizeof(SK);

template <bool HUB>
__global__ __launch_bounds__(64 * kAWaves) void k_atac_port(AtacDev D, AtacPk K, const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ ids, SK* scr)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t alds[];
  const NocParams& P = D.P;
  const uint32_t ln = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t g = HUB ? blockIdx.x : blockIdx.x * kAWaves + wv;   // AP: tile; HUB: cluster
  if (g >= (HUB ? D.C : P.tiles)) return;
  const uint64_t b = off[g], e = off[g + 1];
  if (b == e) return;
  const uint32_t n = (uint32_t)(e - b);
  auto fill = [&](uint32_t i) { const uint32_t k = ids[b + i]; return SK{K.t[k], k, k}; };
  const SK* A = HUB ? block_sorted(reinterpret_cast<SK*>(alds), kAWaves * kAPk, scr + b, n, fill)
                    : wave_sorted(reinterpret_cast<SK*>(alds) + (size_t)wv * kAPk, kAPk, scr + b, n, ln, fill);
  if (HUB && wv != 0) return;
  const uint64_t qi = HUB ? (uint64_t)P.tiles + g : (uint64_t)g;
  WaveQueue Q;
  Q.open(P, D.q + qi, D.nd + qi * P.max_size, ln);
  const uint32_t owner = HUB ? D.hub_of[g] : g;                  // the tile that owns the component
  const uint64_t zps = lat_to_ps(HUB ? (uint64_t)D.A.send_hub_router_delay + 3 : (uint64_t)D.A.enet_router_delay + 1, P.f);
  const bool bc_laser = (D.A.laser_modes & GG_ATAC_LASER_BROADCAST) != 0, uni_laser = (D.A.laser_modes & GG_ATAC_LASER_UNICAST) != 0;
  uint64_t cq = 0;                                               // uniform: the port's contention cycles
  uint64_t sf = 0, sreq = 0, ouni = 0, obc = 0;                  // this lane's requests: flits, count, optical flits
  for (uint32_t j0 = 0; j0 < n; j0 += 64) {
    const uint32_t cnt = min(64u, n - j0);
    const bool mine = ln < cnt;
    const uint32_t k = mine ? A[j0 + ln].i : 0u;
    const uint64_t myt = mine ? A[j0 + ln].t : 0;
    const uint32_t bits = mine ? K.len[k] : 0u;
    const uint32_t mynf = mine ? (uint32_t)nflits(P, bits) : 0u;
    const uint64_t myzl = mine ? K.zl[k] : 0, myct = mine ? K.ct[k] : 0;
    const uint32_t myb = (HUB && mine && K.route[k] == R_BCAST) ? K.bidx[k] : ~0u;
    uint64_t qmine = 0;
    for (uint32_t j = 0; j < cnt; ++j) {
      const uint64_t t = rl64(myt, j);
      const uint32_t nf = rl32(mynf, j);
      const uint64_t cyc = time_to_cycles(t, P.f);
      const uint32_t bj = HUB ? rl32(myb, j) : ~0u;
      if (HUB && bj != ~0u && !bc_laser) {
        // a broadcast under a unicast-only laser: one request per cluster at
        // the same packet time, each copy with its own delay (:447-461)
        const uint64_t zl = rl64(myzl, j), ct = rl64(myct, j);
        for (uint32_t c = 0; c < D.C; ++c) {
          const uint64_t qd = Q.request(cyc, nf, D.err);
          cq += qd;
          if (ln == 0) {
            const uint64_t r = (uint64_t)K.n + (uint64_t)bj * D.C + c, cps = lat_to_ps(qd, P.f);
            K.rt[r] = t + zps + cps; K.rzl[r] = zl + zps; K.rct[r] = ct + cps;
          }
        }
      } else {
        const uint64_t qd = Q.request(cyc, nf, D.err);
        cq += qd;
        if (ln == j) qmine = qd;
      }
    }
    if (mine) {
      const uint64_t cps = lat_to_ps(qmine, P.f);
      const uint64_t t2 = myt + zps + cps, z2 = myzl + zps, c2 = myct + cps;
      if (!HUB) { K.t[k] = t2; K.zl[k] = z2; K.ct[k] = c2; sf += mynf; sreq += 1; }
      else if (myb == ~0u) {                                     // a unicast to the receiver's hub
        K.rt[k] = t2; K.rzl[k] = z2; K.rct[k] = c2;
        sf += mynf; sreq += 1;
        if (uni_laser) ouni += mynf; else obc += mynf;           // optical_link_model.cc:121-134
      } else if (bc_laser) {                                     // one request, a copy per cluster (:433-446)
        for (uint32_t c = 0; c < D.C; ++c) {
          const uint64_t r = (uint64_t)K.n + (uint64_t)myb * D.C + c;
          K.rt[r] = t2; K.rzl[r] = z2; K.rct[r] = c2;
        }
        sf += mynf; sreq += 1; obc += mynf;
      } else { sf += (uint64_t)mynf * D.C; sreq += D.C; ouni += (uint64_t)mynf * D.C; }
    }
  }
  Q.close();
  sf = wave_sum64n(sf); sreq = wave_sum64n(sreq); ouni = wave_sum64n(ouni); obc = wave_sum64n(obc);
  if (ln == 0) {
    if (!HUB) {                                                  // the ENet router's sixth port and its link
      if (P.qm) { cadd(D.ctr, owner, GG_NC_ROUTER_CONTENTION_CYCLES, cq); cadd(D.ctr, owner, GG_NC_ROUTER_PACKETS, sreq); }
      cadd(D.ctr, owner, GG_NC_BUFFER_WRITES, sf); cadd(D.ctr, owner, GG_NC_BUFFER_READS, sf);
      cadd(D.ctr, owner, GG_NC_SWITCH_ALLOC, sreq); cadd(D.ctr, owner, GG_NC_CROSSBAR, sf);
      cadd(D.ctr, owner, GG_NC_LINK_TRAVERSALS, sf);
    } else {
      const int R = GG_AC_SEND_HUB;
      if (P.qm) { aadd(D.actr, owner, R + GG_ACR_CONTENTION_CYCLES, cq); aadd(D.actr, owner, R + GG_ACR_PORT_PACKETS, sreq); }
      aadd(D.actr, owner, R + GG_ACR_BUFFER_WRITES, sf); aadd(D.actr, owner, R + GG_ACR_SWITCH_ALLOC, sreq);
      aadd(D.actr, owner, R + GG_ACR_CROSSBAR_ONE, sf);
      aadd(D.actr, owner, GG_AC_OPTICAL_UNICAST_FLITS, ouni); aadd(D.actr, owner, GG_AC_OPTICAL_BROADCAST_FLITS, obc);
    }
  }
}

// ---------------------------------------------------------------------------
// Receive stage: one workgroup per (cluster, receive net).  Its events — the
// unicasts for the cluster's tiles and one copy of every broadcast, from the
// senders whose cluster maps to this net — sorted by (time, packet index) in
// LDS; task 0 = the receive hub's output port of the net, task 1 + p = port p
// of the net's star router, a wave per task (tasks beyond 16 waves wrap).  A
// task walks the sorted events and serves those that ask its queue: the hub
// port all of them, a star port the unicasts to its tile and every broadcast.
// A broadcast's star delay is the largest over the ports.  Then the threads
// turn events into deliveries; the receivers are the cluster's own tiles, so
// their counters gather in LDS.
// ---------------------------------------------------------------------------
constexpr uint32_t kRPk = 8192, kRMaxWaves = 16;
constexpr uint32_t kRAcc = 5;                                    // a tile's receive counters
constexpr size_t kRLds = (size_t)kRPk * sizeof(SK);

__global__ __launch_bounds__(64 * kRMaxWaves) void k_atac_receive(AtacDev D, AtacPk K, const uint64_t* __restrict__ off,
    const uint32_t* __restrict__ ids, SK* scr, uint64_t* dhub, unsigned long long* dstar)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t rlds[];
  __shared__ unsigned long long racc[GG_ATAC_MAX_STAR_PORTS * kRAcc];
  __shared__ unsigned long long hacc[16];
  const NocParams& P = D.P;
  const uint32_t g = blockIdx.x, cl = g / D.A.num_receive_nets;
  const uint64_t b = off[g], e = off[g + 1];
  if (b == e) return;
  const uint32_t n = (uint32_t)(e - b), tid = threadIdx.x, ln = tid & 63, wv = tid >> 6, nwv = blockDim.x >> 6;
  const uint32_t cs = D.A.cluster_size;
  const bool star = D.A.receive_net_type == GG_ATAC_STAR;
  for (uint32_t i = tid; i < GG_ATAC_MAX_STAR_PORTS * kRAcc; i += blockDim.x) racc[i] = 0;
  if (tid < 16) hacc[tid] = 0;
  // ---- sort
  const SK* A = block_sorted(reinterpret_cast<SK*>(rlds), kRPk, scr + b, n, [&](uint32_t i) {
    const uint32_t r = ids[b + i];
    const uint32_t k = r < K.n ? r : K.bpkt[(r - K.n) / D.C];
    return SK{K.rt[r], k, r};
  });
  // ---- serve: a wave per queue
  const uint32_t ntasks = star ? 1 + cs : 1;
  for (uint32_t task = wv; task < ntasks; task += nwv) {
    const uint64_t qi = task == 0 ? D.rh0() + g : D.st0() + (uint64_t)g * cs + (task - 1);
    WaveQueue Q;
    Q.open(P, D.q + qi, D.nd + qi * P.max_size, ln);
    if (!Q.on) break;                                            // no contention model: no delays
    for (uint32_t j0 = 0; j0 < n; j0 += 64) {
      const uint32_t cnt = min(64u, n - j0);
      const bool mine = ln < cnt;
      const uint32_t k = mine ? A[j0 + ln].i : 0u;
      const uint64_t myt = mine ? A[j0 + ln].t : 0;
      const uint32_t mynf = mine ? (uint32_t)nflits(P, K.len[k]) : 0u;
      const uint32_t d = mine ? K.dst[k] : 0u;
      // the star port the event asks: its receiver's index in the cluster, or all (a broadcast)
      const uint32_t myport = !mine ? ~1u : d == GG_BROADCAST ? ~0u : D.star_of[d];
      uint64_t qmine = 0;
      for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t pj = rl32(myport, j);
        if (task != 0 && pj != ~0u && pj != task - 1) continue;
        const uint64_t qd = Q.request(time_to_cycles(rl64(myt, j), P.f), rl32(mynf, j), D.err);
        if (ln == j) qmine = qd;
      }
      if (mine) {
        if (task == 0) dhub[b + j0 + ln] = qmine;
        else if (myport == ~0u) atomicMax(&dstar[b + j0 + ln], (unsigned long long)qmine);
        else if (myport == task - 1) dstar[b + j0 + ln] = qmine;
      }
    }
    Q.close();
  }
  __threadfence();
  __syncthreads();
  // ---- deliver
  const uint64_t zps = lat_to_ps((uint64_t)D.A.receive_hub_router_delay + (star ? (uint64_t)D.A.star_net_router_delay + 1 : 1ull), P.f);
  // hub-tile counters of this thread's events: receive hub (flits, requests, contention), star (flits one / all,
  // requests, contention, port packets), receive-net link flits
  uint64_t hf = 0, hn = 0, hc = 0, s1 = 0, sa = 0, sn = 0, sc = 0, sp = 0, lk = 0;
  for (uint32_t j = tid; j < n; j += blockDim.x) {
    const SK ev = A[j];
    const uint32_t k = ev.i, r = ev.pad, bits = K.len[k], d = K.dst[k];
    const uint64_t nf = nflits(P, bits);
    const uint64_t qh = P.qm ? dhub[b + j] : 0, qs = (P.qm && star) ? (uint64_t)dstar[b + j] : 0;
    const bool bc = d == GG_BROADCAST;
    const uint32_t np = bc ? cs : 1u;                            // star ports asked / receivers
    hf += nf; hn += 1; hc += qh;
    if (star) {
      if (np == 1) s1 += nf; else sa += nf;
      sn += 1; sc += qs * np; sp += np; lk += nf * np;
    } else lk += nf;
    const uint64_t cps = lat_to_ps(qh + qs, P.f), ser = lat_to_ps(nf, P.f);
    const uint64_t t2 = ev.t + zps + cps + ser, z2 = K.rzl[r] + zps + ser, c2 = K.rct[r] + cps;
    for (uint32_t i = 0; i < np; ++i) {
      const uint32_t idx = bc ? i : D.star_of[d];
      if (bc) {
        const uint64_t o = (uint64_t)K.bidx[k] * P.tiles + D.members[(uint64_t)cl * cs + i];
        K.bout.arrival_ps_dev[o] = t2; K.bout.zero_load_ps_dev[o] = z2; K.bout.contention_ps_dev[o] = c2;
      } else {
        K.out.arrival_ps_dev[k] = t2; K.out.zero_load_ps_dev[k] = z2; K.out.contention_ps_dev[k] = c2;
      }
      unsigned long long* a = racc + idx * kRAcc;
      atomicAdd(a + 0, 1ull); atomicAdd(a + 1, (unsigned long long)nf); atomicAdd(a + 2, (unsigned long long)bits);
      atomicAdd(a + 3, (unsigned long long)(z2 + c2)); atomicAdd(a + 4, (unsigned long long)c2);
    }
  }
  uint64_t v[9] = {hf, hn, hc, s1, sa, sn, sc, sp, lk};
  #pragma unroll
  for (int i = 0; i < 9; ++i) { const uint64_t w = wave_sum64n(v[i]); if (ln == 0 && w) atomicAdd(&hacc[i], (unsigned long long)w); }
  __syncthreads();
  for (uint32_t i = tid; i < cs * kRAcc; i += blockDim.x) {
    const uint32_t tile = D.members[(uint64_t)cl * cs + i / kRAcc];
    const int f[kRAcc] = {GG_NC_PACKETS_RECEIVED, GG_NC_FLITS_RECEIVED, GG_NC_BITS_RECEIVED, GG_NC_TOTAL_LATENCY_PS,
                          GG_NC_TOTAL_CONTENTION_PS};
    cadd(D.ctr, tile, f[i % kRAcc], racc[i]);
  }
  if (tid == 0) {
    const uint32_t hub = D.hub_of[cl];
    const int H = GG_AC_RECEIVE_HUB, S = GG_AC_STAR_NET;
    aadd(D.actr, hub, H + GG_ACR_BUFFER_WRITES, hacc[0]); aadd(D.actr, hub, H + GG_ACR_SWITCH_ALLOC, hacc[1]);
    aadd(D.actr, hub, H + GG_ACR_CROSSBAR_ONE, hacc[0]);
    if (P.qm) { aadd(D.actr, hub, H + GG_ACR_CONTENTION_CYCLES, hacc[2]); aadd(D.actr, hub, H + GG_ACR_PORT_PACKETS, hacc[1]); }
    aadd(D.actr, hub, S + GG_ACR_BUFFER_WRITES, hacc[3] + hacc[4]); aadd(D.actr, hub, S + GG_ACR_SWITCH_ALLOC, hacc[5]);
    aadd(D.actr, hub, S + GG_ACR_CROSSBAR_ONE, hacc[3]); aadd(D.actr, hub, S + GG_ACR_CROSSBAR_ALL, hacc[4]);
    if (P.qm) { aadd(D.actr, hub, S + GG_ACR_CONTENTION_CYCLES, hacc[6]); aadd(D.actr, hub, S + GG_ACR_PORT_PACKETS, hacc[7]); }
    aadd(D.actr, hub, GG_AC_RECEIVE_NET_LINK_FLITS, hacc[8]);
  }
}

// the packets that never left the ENet (its SELF stage received them) and the corner cases
__global__ void k_atac_out(AtacPk K)
{
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K.n) return;
  const uint8_t r = K.route[k];
  if (r == R_ENET) {
    K.out.arrival_ps_dev[k] = K.t[k]; K.out.zero_load_ps_dev[k] = K.zl[k]; K.out.contention_ps_dev[k] = K.ct[k];
  } else if (r == R_NONE) {                                      // src == dst: no time, no counters (processCornerCases)
    K.out.arrival_ps_dev[k] = K.t0[k]; K.out.zero_load_ps_dev[k] = 0; K.out.contention_ps_dev[k] = 0;
  }
}

__global__ void k_atac_qreset(HQueue* q, HNode* nd, uint64_t nq, uint32_t max_size, uint32_t type, uint32_t aux)
{
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nq) return;
  hq_init(q + i, nd + i * max_size, max_size, type, aux);
}

bool pow2(uint64_t n) { return n && !(n & (n - 1)); }
uint32_t isqrt(uint64_t n) { uint32_t r = (uint32_t)floor(sqrt((double)n)); while ((uint64_t)r * r > n) --r; while ((uint64_t)(r + 1) * (r + 1) <= n) ++r; return r; }
int flog2(uint64_t n) { int p = -1; while (n) { n >>= 1; ++p; } return p; }

struct Topo { uint32_t W, C, cw, ch, cmw, sw, sh; };

// NetworkModelAtac::initializeANetTopologyParams (:104-121) + initializeClusters (:587-639)
gg_status atac_check(uint32_t T, const gg_atac_params& p, Topo* out)
{
  if (!pow2(T) || (uint64_t)isqrt(T) * isqrt(T) != T)
    return gg_fail(GG_ERR_INVALID, "atac: num_tiles %u must be a power of two and a perfect square", T);
  if (!pow2(p.cluster_size)) return gg_fail(GG_ERR_INVALID, "atac: cluster_size %u must be a power of two", p.cluster_size);
  if (!pow2(p.num_access_points))
    return gg_fail(GG_ERR_INVALID, "atac: num_access_points %u must be a power of two", p.num_access_points);
  if (p.num_access_points > p.cluster_size)
    return gg_fail(GG_ERR_INVALID, "atac: num_access_points %u above cluster_size %u", p.num_access_points, p.cluster_size);
  if (T % p.cluster_size || T / p.cluster_size < 2)
    return gg_fail(GG_ERR_INVALID, "atac: cluster_size %u leaves fewer than 2 clusters of %u tiles", p.cluster_size, T);
  if (p.num_receive_nets == 0) return gg_fail(GG_ERR_INVALID, "atac: num_receive_nets must be at least 1");
  if (p.laser_modes == 0 || p.laser_modes > 3)
    return gg_fail(GG_ERR_INVALID, "atac: laser_modes %u must enable unicast (1), broadcast (2) or both", p.laser_modes);
  if (p.receive_net_type > GG_ATAC_BTREE) return gg_fail(GG_ERR_INVALID, "atac: unknown receive_net_type %u", p.receive_net_type);
  if (p.global_routing > GG_ATAC_DISTANCE_BASED) return gg_fail(GG_ERR_INVALID, "atac: unknown global_routing %u", p.global_routing);
  if (p.cluster_size > GG_ATAC_MAX_STAR_PORTS)
    return gg_fail(GG_ERR_UNSUPPORTED, "atac: cluster_size %u above %u, the ports the star stage holds (a wave per port in "
                   "one workgroup)", p.cluster_size, GG_ATAC_MAX_STAR_PORTS);
  if (p.num_receive_nets > 1024) return gg_fail(GG_ERR_UNSUPPORTED, "atac: num_receive_nets %u above 1024", p.num_receive_nets);
  Topo t;
  t.W = isqrt(T); t.C = T / p.cluster_size;
  auto grid = [](uint32_t n, bool wide, uint32_t& x, uint32_t& y) {
    if (flog2(n) % 2 == 0) { x = y = isqrt(n); return; }
    const uint32_t a = isqrt(n / 2), b = isqrt((uint64_t)n * 2);
    x = wide ? b : a; y = wide ? a : b;
  };
  uint32_t nx, ny, sx, sy;
  grid(t.C, false, nx, ny);                       // clusters: X = sqrt(C / 2), Y = sqrt(2 C) when log2 C is odd
  t.cw = t.W / nx; t.ch = t.W / ny; t.cmw = t.W / t.cw;
  grid(p.num_access_points, true, sx, sy);        // sub-clusters: the other way round
  t.sw = t.cw / sx; t.sh = t.ch / sy;
  if (t.sw == 0 || t.sh == 0)
    return gg_fail(GG_ERR_INVALID, "atac: num_access_points %u does not tile a %u x %u cluster", p.num_access_points, t.cw, t.ch);
  if (out) *out = t;
  return GG_OK;
}

void atac_topology(uint32_t T, const gg_atac_params& p, const Topo& t, uint32_t* cluster, uint32_t* ap, uint32_t* hub,
                   uint32_t* star, uint32_t* members)
{
  for (uint32_t i = 0; i < T; ++i) {
    const uint32_t x = i % t.W, y = i / t.W;
    const uint32_t c = (y / t.ch) * t.cmw + x / t.cw;                           // getClusterID (:659-674)
    const uint32_t minx = (c % t.cmw) * t.cw, miny = (c / t.cmw) * t.ch;
    const uint32_t si = (x - minx) * t.ch + (y - miny);                         // getTileIDListInCluster (:722-745)
    if (cluster) cluster[i] = c;
    if (ap) ap[i] = (miny + ((y - miny) / t.sh) * t.sh + t.sh / 2) * t.W + minx + ((x - minx) / t.sw) * t.sw + t.sw / 2;
    if (star) star[i] = si;
    if (members) members[(size_t)c * p.cluster_size + si] = i;
  }
  if (hub)
    for (uint32_t c = 0; c < t.C; ++c)                                          // getTileIDWithOpticalHub (:704-720)
      hub[c] = ((c / t.cmw) * t.ch + t.ch / 2) * t.W + (c % t.cmw) * t.cw + t.cw / 2;
}

}  // namespace

struct gg_atac_state {
  gg_atac_params A{};
  uint32_t C = 0;
  uint64_t nq = 0;
  gg_arena mem;            // owns the topology tables, q, nd and actr
  uint32_t *cluster_of = nullptr, *ap_of = nullptr, *hub_of = nullptr, *star_of = nullptr, *members = nullptr;
  HQueue* q = nullptr; HNode* nd = nullptr;
  uint64_t* actr = nullptr;
  // batch scratch: the per-packet arrays share one capacity, the per-record arrays another
  gg_dbuf<uint8_t> route;
  gg_dbuf<uint32_t> dinj, dxy, dself, bidx, bpkt, nbc;
  gg_dbuf<uint64_t> rt, rzl, rct, dhub, dstar;
  gg_dbuf<uint32_t> keys, ids;
  gg_dbuf<SK> scr;
  gg_dbuf<uint32_t> counts, cursor; gg_dbuf<uint64_t> off;
};

void gg_atac_free(gg_ctx* ctx)
{
  delete ctx->atac;
  ctx->atac = nullptr;
}

// (re)builds the ATAC state of the context for params p (NULL: the defaults); the caller resets the NoC state
gg_status gg_atac_alloc(gg_ctx* ctx, const gg_atac_params* p)
{
  gg_atac_params A;
  if (p) A = *p; else gg_atac_params_default(&A);
  const uint32_t T = ctx->cfg.num_tiles;
  Topo t;
  if (gg_status st = atac_check(T, A, &t)) return st;
  gg_atac_free(ctx);
  gg_atac_state* S = new gg_atac_state();
  ctx->atac = S;
  S->A = A; S->C = t.C;
  const NocParams P = gg_noc_params(ctx);
  std::vector<uint32_t> cl(T), ap(T), hub(t.C), star(T), mem(T);
  atac_topology(T, A, t, cl.data(), ap.data(), hub.data(), star.data(), mem.data());
  auto up = [&](uint32_t** d, const std::vector<uint32_t>& h) -> gg_status {
    if (gg_status st = S->mem.alloc(d, h.size())) return st;
    GG_HIP(hipMemcpy(*d, h.data(), 4 * h.size(), hipMemcpyHostToDevice));
    return GG_OK;
  };
  if (gg_status st = up(&S->cluster_of, cl)) return st;
  if (gg_status st = up(&S->ap_of, ap)) return st;
  if (gg_status st = up(&S->hub_of, hub)) return st;
  if (gg_status st = up(&S->star_of, star)) return st;
  if (gg_status st = up(&S->members, mem)) return st;
  const uint64_t G = (uint64_t)t.C * A.num_receive_nets;
  S->nq = (uint64_t)T + t.C + G * (1 + (A.receive_net_type == GG_ATAC_STAR ? A.cluster_size : 0));
  if (gg_status st = S->mem.alloc(&S->q, S->nq)) return st;
  if (gg_status st = S->mem.alloc(&S->nd, S->nq * P.max_size)) return st;
  if (gg_status st = S->mem.alloc(&S->actr, (uint64_t)T * GG_NUM_ATAC_COUNTERS)) return st;
  GG_HIP(hipFuncSetAttribute((const void*)k_atac_port<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kALds));
  GG_HIP(hipFuncSetAttribute((const void*)k_atac_port<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kALds));
  GG_HIP(hipFuncSetAttribute((const void*)k_atac_receive, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRLds));
  gg_noc_set_enet(ctx, A.enet_router_delay);
  return GG_OK;
}

gg_status gg_atac_reset(gg_ctx* ctx, hipStream_t s)
{
  gg_atac_state* S = ctx->atac;
  if (!S) return GG_OK;
  const NocParams P = gg_noc_params(ctx);
  GG_HIP(hipMemsetAsync(S->actr, 0, sizeof(uint64_t) * P.tiles * GG_NUM_ATAC_COUNTERS, s));
  hipLaunchKernelGGL(k_atac_qreset, dim3((uint32_t)((S->nq + 255) / 256)), dim3(256), 0, s, S->q, S->nd, S->nq, P.max_size,
                     P.qtype, P.qaux);
  GG_HIP(hipGetLastError());
  return GG_OK;
}

static gg_status atac_grow(gg_atac_state* S, uint64_t n, uint64_t nrec, uint64_t nbc, uint32_t nbuckets)
{
  if (gg_status st = gg_reserve_all(n, n + n / 4 + 1024, S->route, S->dinj, S->dxy, S->dself, S->bidx)) return st;
  if (gg_status st = gg_reserve_all(nrec, nrec + nrec / 4 + 1024, S->rt, S->rzl, S->rct, S->dhub, S->dstar, S->keys, S->ids,
                                    S->scr))
    return st;
  if (gg_status st = S->bpkt.reserve(nbc + 1, nbc + 1024)) return st;
  if (gg_status st = S->nbc.reserve(1)) return st;
  return gg_reserve_all((uint64_t)nbuckets + 1, (uint64_t)nbuckets + 1, S->counts, S->cursor, S->off);   // one size per state
}

gg_status gg_atac_run(gg_ctx* ctx, const gg_packets* pk, const gg_packet_out* out, const gg_packet_out* bout, uint64_t nb,
                      hipStream_t s)
{
  gg_atac_state* S = ctx->atac;
  if (!S) return gg_fail(GG_ERR_STATE, "atac: no ATAC state");
  const NocParams P = gg_noc_params(ctx);
  const uint64_t n = pk->num_packets;
  if (n == 0) return GG_OK;
  if (!pk->src_dev || !pk->dst_dev || !pk->length_bits_dev || !pk->time_ps_dev ||
      !out->arrival_ps_dev || !out->zero_load_ps_dev || !out->contention_ps_dev ||
      (nb && (!bout || !bout->arrival_ps_dev || !bout->zero_load_ps_dev || !bout->contention_ps_dev)))
    return gg_fail(GG_ERR_INVALID, "NULL packet or output pointer");
  const uint64_t nrec = n + nb * S->C;
  if (n >= (1ull << 32) || nb > n || nrec >= (1ull << 32))
    return gg_fail(GG_ERR_RANGE, "batch larger than 2^32 packets or broadcast copies, or num_broadcasts > packets");
  const uint32_t G = S->C * S->A.num_receive_nets;                 // receive buckets
  const uint32_t nbuckets = std::max(P.tiles, G);
  if (gg_status st = atac_grow(S, n, nrec, nb, nbuckets)) return st;
  AtacDev D{P, S->A, S->C, S->cluster_of, S->ap_of, S->hub_of, S->star_of, S->members, S->q, S->nd, gg_noc_ctr(ctx), S->actr,
            ctx->err_dev};
  const gg_packet_out none{nullptr, nullptr, nullptr};
  AtacPk K{pk->src_dev, pk->dst_dev, pk->length_bits_dev, pk->time_ps_dev, (uint32_t)n, nb, S->route, S->dinj, S->dxy, S->dself,
           S->bidx, S->bpkt, S->nbc, nullptr, nullptr, nullptr, S->rt, S->rzl, S->rct, *out, nb ? *bout : none};
  const uint32_t pblocks = (uint32_t)((n + 255) / 256), rblocks = (uint32_t)((nrec + 255) / 256);
  gg_timer_begin(ctx, "noc_atac", s);
  hipLaunchKernelGGL(k_atac_bscan, dim3(1), dim3(1024), 0, s, D, K);
  hipLaunchKernelGGL(k_atac_prep, dim3(pblocks), dim3(256), 0, s, D, K);
  GG_HIP(hipGetLastError());
  // ENet: injection, X, Y and (ENet packets) the SELF port + receive
  gg_timer_begin(ctx, "noc_atac_enet", s);
  if (gg_status st = gg_noc_enet_stages(ctx, K.src, K.dinj, K.dxy, K.dself, K.len, K.t0, n, s)) return st;
  gg_timer_end(ctx, "noc_atac_enet", s);
  gg_noc_packet_state(ctx, &K.t, &K.zl, &K.ct);                   // (re)allocated by the stages
  auto bucket = [&](int stage, uint32_t nbk) -> gg_status {
    GG_HIP(hipMemsetAsync(S->counts, 0, 4 * ((uint64_t)nbk + 1), s));
    if (stage == 0) hipLaunchKernelGGL(k_atac_keys<0>, dim3(pblocks), dim3(256), 0, s, D, K, n, S->keys, S->counts);
    else if (stage == 1) hipLaunchKernelGGL(k_atac_keys<1>, dim3(pblocks), dim3(256), 0, s, D, K, n, S->keys, S->counts);
    else hipLaunchKernelGGL(k_atac_keys<2>, dim3(rblocks), dim3(256), 0, s, D, K, nrec, S->keys, S->counts);
    hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, S->counts, nbk, S->off, S->cursor);
    const uint64_t m = stage == 2 ? nrec : n;
    hipLaunchKernelGGL(k_bucket, dim3((uint32_t)((m + 255) / 256)), dim3(256), 0, s, S->keys, m, nullptr, S->off, S->cursor, S->ids);
    GG_HIP(hipGetLastError());
    return GG_OK;
  };
  gg_timer_begin(ctx, "noc_atac_access_point", s);
  if (gg_status st = bucket(0, P.tiles)) return st;
  hipLaunchKernelGGL(k_atac_port<false>, dim3((P.tiles + kAWaves - 1) / kAWaves), dim3(64 * kAWaves), kALds, s, D, K, S->off,
                     S->ids, S->scr);
  gg_timer_end(ctx, "noc_atac_access_point", s);
  gg_timer_begin(ctx, "noc_atac_send_hub", s);
  if (gg_status st = bucket(1, S->C)) return st;
  hipLaunchKernelGGL(k_atac_port<true>, dim3(S->C), dim3(64 * kAWaves), kALds, s, D, K, S->off,
                     S->ids, S->scr);
  gg_timer_end(ctx, "noc_atac_send_hub", s);
  gg_timer_begin(ctx, "noc_atac_receive", s);
  if (gg_status st = bucket(2, G)) return st;
  const bool star = S->A.receive_net_type == GG_ATAC_STAR;
  if (star && P.qm) GG_HIP(hipMemsetAsync(S->dstar, 0, 8 * nrec, s));   // a broadcast's star delay: the max over the ports
  const uint32_t waves = std::min<uint32_t>(kRMaxWaves, star && P.qm ? 1 + S->A.cluster_size : 4u);
  hipLaunchKernelGGL(k_atac_receive, dim3(G), dim3(64 * waves), kRLds, s, D, K, S->off, S->ids, S->scr, S->dhub,
                     reinterpret_cast<unsigned long long*>(S->dstar.get()));
  gg_timer_end(ctx, "noc_atac_receive", s);
  hipLaunchKernelGGL(k_atac_out, dim3(pblocks), dim3(256), 0, s, K);
  GG_HIP(hipGetLastError());
  gg_timer_end(ctx, "noc_atac", s);
  return GG_OK;
}

extern "C" {

void gg_atac_params_default(gg_atac_params* p)
{
  if (!p) return;
  p->cluster_size = 4; p->num_access_points = 4;                    /* carbon_sim.cfg:318-327 */
  p->receive_net_type = GG_ATAC_STAR; p->num_receive_nets = 2;
  p->global_routing = GG_ATAC_CLUSTER_BASED; p->unicast_distance_threshold = 4;
  p->enet_router_delay = 1; p->send_hub_router_delay = 1;           /* :329-348 */
  p->receive_hub_router_delay = 1; p->star_net_router_delay = 1;
  p->laser_modes = GG_ATAC_LASER_UNICAST | GG_ATAC_LASER_BROADCAST; /* :366-370 */
}

gg_status gg_noc_set_atac(gg_ctx* ctx, const gg_atac_params* p)
{
  if (!ctx || !p) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (ctx->cfg.net_model != GG_NET_ATAC)
    return gg_fail(GG_ERR_INVALID, "gg_noc_set_atac: net_model %u is not GG_NET_ATAC", ctx->cfg.net_model);
  hipSetDevice(ctx->device);
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  if (gg_status st = gg_atac_alloc(ctx, p)) return st;             // a rejected p leaves the context as it was
  return gg_reset(ctx);
}

gg_status gg_atac_topology(uint32_t num_tiles, const gg_atac_params* p, uint32_t* cluster_of, uint32_t* access_point_of,
                           uint32_t* hub_of_cluster, uint32_t* star_index_of)
{
  if (!p) return gg_fail(GG_ERR_INVALID, "NULL argument");
  Topo t;
  if (gg_status st = atac_check(num_tiles, *p, &t)) return st;
  atac_topology(num_tiles, *p, t, cluster_of, access_point_of, hub_of_cluster, star_index_of, nullptr);
  return GG_OK;
}

gg_status gg_noc_get_atac_counters(gg_ctx* ctx, uint64_t* out)
{
  if (!ctx || !out) return gg_fail(GG_ERR_INVALID, "NULL argument");
  if (ctx->cfg.net_model != GG_NET_ATAC || !ctx->atac)
    return gg_fail(GG_ERR_INVALID, "gg_noc_get_atac_counters: net_model %u is not GG_NET_ATAC", ctx->cfg.net_model);
  hipSetDevice(ctx->device);
  GG_HIP(hipStreamSynchronize(ctx->last_stream));
  const uint32_t T = ctx->cfg.num_tiles;
  GG_HIP(hipMemcpy(out, ctx->atac->actr, sizeof(uint64_t) * T * GG_NUM_ATAC_COUNTERS, hipMemcpyDeviceToHost));
  // the ENet router (its sixth port included) counts in the mesh router's fields of the NoC counters
  std::vector<uint64_t> nc((size_t)T * GG_NUM_NET_COUNTERS);
  GG_HIP(hipMemcpy(nc.data(), gg_noc_ctr(ctx), sizeof(uint64_t) * nc.size(), hipMemcpyDeviceToHost));
  for (uint32_t t = 0; t < T; ++t) {
    const uint64_t* c = nc.data() + (size_t)t * GG_NUM_NET_COUNTERS;
    uint64_t* a = out + (size_t)t * GG_NUM_ATAC_COUNTERS;
    a[GG_AC_ENET + GG_ACR_BUFFER_WRITES] = c[GG_NC_BUFFER_WRITES]; a[GG_AC_ENET + GG_ACR_SWITCH_ALLOC] = c[GG_NC_SWITCH_ALLOC];
    a[GG_AC_ENET + GG_ACR_CROSSBAR_ONE] = c[GG_NC_CROSSBAR]; a[GG_AC_ENET + GG_ACR_CROSSBAR_ALL] = 0;
    a[GG_AC_ENET + GG_ACR_CONTENTION_CYCLES] = c[GG_NC_ROUTER_CONTENTION_CYCLES];
    a[GG_AC_ENET + GG_ACR_PORT_PACKETS] = c[GG_NC_ROUTER_PACKETS];
    a[GG_AC_ENET_LINK_FLITS] = c[GG_NC_LINK_TRAVERSALS];
  }
  return GG_OK;
}

}  // extern "C"
